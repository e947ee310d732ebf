"""The cases of tests/test_gpu_sequences.py are what that file takes them for, by the plain reference loops alone: the plan
workgroups each one fills, no error in the good ones, HBS_E_ARG with the edited entry named in the malformed ones, HBS_E_CAPACITY
in the ones a byte short.  The same for the RTP and MP4 calls of tests/test_gpu_sequences_rtp_mp4.py (S.CALLS2), with the output
tiles, a variant for each capacity that is one short, the roomy variants and the pipelines' later stages.  No GPU."""
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


# ---- the RTP and MP4 calls (S.CALLS2) ---------------------------------------------------------------------------------------------

TILED = dict(rtp="out", rtpa="out", rtpu="out", mp4f="out")          # the calls that copy by output tiles of S.TILE bytes
# what the header promises of the counts under HBS_E_CAPACITY, where it is not "the counts are right"
RIGHT_WHEN_SHORT = {("rtpo", "short_span"): ("nal_found", "stream_bytes"), ("mp4s", "short_moof"): ("nal_found",),
                    ("mp4s", "short_sample"): ("nal_count", "nal_found"), ("stbl", "short_sample"): ("nal_count", "nal_found")}


@pytest.mark.parametrize("call", S.CALLS2)
def test_plan_workgroups_and_tiles_of_every_rtp_and_mp4_case(call):
    small, large, odd = (S.case(call, w) for w in S.SIZES)
    assert all(b == 1 for b in S.plan_blocks(small)), (small, S.items(small))
    for n, per in S.items(large):
        assert per == 256 and S.blocks(n, per) >= 3 and n % per, (large, n, per)
    for lo, mid, hi in zip(S.plan_blocks(small), S.plan_blocks(odd), S.plan_blocks(large)):
        assert lo < mid < hi, (odd, S.items(odd), S.items(large))
    assert all(n == 0 for n, _ in S.items(S.empty(call)))
    if call in TILED:                              # three output tiles and more; one in the small case
        assert S.blocks(large.room[TILED[call]], S.TILE) >= 3 and S.blocks(small.room[TILED[call]], S.TILE) <= 2
    if call == "rtpa":                             # aggregation packets in every case, most NALs in one
        for c in (small, large, odd):
            assert S.summary_of(c)["reserved"][2] >> 32 > len(c.a["index"]) // 8
    if call == "rtp":
        assert all(S.summary_of(c)["reserved"][2] > len(c.a["index"]) // 8 for c in (small, large, odd))          # NALs sent as FUs
    if call == "rtpo":                             # more than three workgroups of slots; packets displaced across workgroups
        assert large.a["prm"]["max_span"] > 3 * S.RTPO_BLOCK and small.a["prm"]["max_span"] == S.RTPO_BLOCK
        assert S.summary_of(large)["reserved"][2] & 0xFFFFFFFF > 2 * S.RTPO_BLOCK
        assert all(S.summary_of(c)["reserved"][1] > 0 and S.summary_of(c)["reserved"][2] >> 32 > 0 for c in (small, large, odd))
    if call == "mp4s":
        assert S.summary_of(large)["nal_found"] > 256 and S.summary_of(large)["nal_count"] > 768
        assert small.a["segs"] is None and large.a["segs"] is None and 1 < len(odd.a["segs"]) <= S.MP4RD_BLOCK
    for c in (small, large, odd):                  # outputs of a few MB at the most, none of them empty
        assert all(0 < n < (4 << 20) for n in c.room.values()), (c, c.room)


@pytest.mark.parametrize("call", S.CALLS2)
def test_the_odd_rtp_and_mp4_case_differs(call):
    small, large, odd = (S.case(call, w).a for w in S.SIZES)
    if call in ("rtp", "rtpa"):
        for k in ("framing", "max_payload", "flags"):
            assert odd["prm"][k] != small["prm"][k] == large["prm"][k], k
        assert odd["pts"] is None and small["pts"] is not None and large["pts"] is not None
    elif call == "rtpu":
        assert odd["prm"]["startcode_bytes"] == 3 and small["prm"]["startcode_bytes"] == large["prm"]["startcode_bytes"] == 4
        assert odd["prm"]["flags"] != small["prm"]["flags"] == large["prm"]["flags"]
        kinds = lambda a: {S.RU.classify(a["data"][int(o):int(o) + int(n)].tobytes(), a["prm"])[0] for o, n in zip(a["off"], a["size"])}          # noqa: E731
        assert S.RU.AP in kinds(odd) and S.RU.AP not in kinds(small) | kinds(large) and S.RU.FU in kinds(small) & kinds(large) & kinds(odd)
    elif call == "rtpo":
        assert odd["prm"]["flags"] == S.RO.AFTER | S.RO.MATCH_SSRC and small["prm"]["flags"] == large["prm"]["flags"] == 0
        s = S.summary_of(S.case(call, "odd"))
        assert s["nal_found"] - s["nal_count"] - (s["reserved"][2] >> 32) == S.RTPO_LATE          # the late packets
    elif call == "mp4f":
        for k in ("length_size", "flags", "max_samples"):
            assert odd["prm"][k] != small["prm"][k] == large["prm"][k], k
        assert odd["dts"] is not None and odd["pts"] is not None and small["dts"] is None and large["dts"] is None
    elif call == "mp4s":
        assert odd["segs"] is not None and odd["stride"] != small["stride"] == large["stride"] and odd["prm"] != small["prm"] == large["prm"]
    elif call == "stbl":
        assert odd["co64"] and not small["co64"] and not large["co64"] and odd["rec"]["flags"][0] == S.MS.CO64
        assert int(odd["rec"]["stss"][0][1]) == 0 and int(small["rec"]["stss"][0][1]) > 0 and int(large["rec"]["stss"][0][1]) > 0
        assert int(odd["rec"]["stsz"][0][1]) == 12 and int(large["rec"]["stsz"][0][1]) == 12 + 4 * len(large["t"]["sizes"])
    else:
        assert odd["params"].get("co64") and odd["params"].get("max_chunk_samples") and not small["params"].get("co64")
        assert not small["params"].get("max_chunk_samples") and small["params"].keys() == large["params"].keys()


@pytest.mark.parametrize("call", S.CALLS2)
def test_good_rtp_and_mp4_cases_and_the_empty_one_have_no_error(call):
    for c in [S.case(call, w) for w in S.SIZES] + [S.empty(call)]:
        for plan in (True, False):
            s = S.summary_of(c, plan)
            assert s["error"] == 0 and s["reserved"][0] == 0, (c, plan, s)
        out = S.want(c)[:-1]
        assert len(out) == len(c.room) and all(x is not None for x in out), c
        for x, room in zip(out, c.room.values()):  # (c.room is in the order of the reference's results)
            assert np.ascontiguousarray(x).view(np.uint8).size == room, (c, room)
    s = S.summary_of(S.empty(call))
    assert s["nal_count"] == 0 and s["nal_found"] == 0 and s["rbsp_bytes"] == 0 and s["reserved"] == [0, 0, 0], s


@pytest.mark.parametrize("call", S.CALLS2)
def test_malformed_rtp_and_mp4_variants_name_their_entry(call):
    for which in S.SIZES:
        good = S.case(call, which)
        for what in ("bad_early", "bad_late"):
            v = S.variant(good, what)
            n, per = v.among
            if what == "bad_early":
                assert 0 <= v.bad < min(per, n), (v, v.bad)
            else:
                assert (S.blocks(n, per) - 1) * per <= v.bad < n, (v, v.bad, v.among)
            word, value = v.named
            assert value == v.bad + 1 or (call == "stbl" and what == "bad_late" and (word, value) == (0, 3)), (v, v.named)
            assert word == 0 or not S.names_the_entry(call) or call == "mp4s"
            for plan in (True, False):             # an argument error shows in a plan as well, where the header has the plan look for it
                s = S.summary_of(v, plan)
                if plan and not v.in_plan:
                    assert s["error"] == 0 and call == "stbl" and what == "bad_early", (v, s)
                    continue
                assert s["error"] == S.E_ARG and s["reserved"][word] == value, (v, plan, s)
                assert all(x == 0 for k, x in enumerate(s["reserved"]) if k != word), (v, plan, s)
            assert all(len(x) == 0 for x in S.want(v)[:-1] if x is not None), v


@pytest.mark.parametrize("call", S.CALLS2)
def test_short_rtp_and_mp4_variants_lack_capacity(call):
    for which in S.SIZES:
        good = S.case(call, which)
        for what in S.SHORTS[call]:
            v = S.variant(good, what)
            s = S.summary_of(v)
            assert s["error"] == S.E_CAPACITY, (v, s)
            if what == "short_span":
                assert v.a["prm"]["max_span"] == S.summary_of(good)["stream_bytes"] - 1 and v.caps == good.caps
            else:
                cap = S.SHORT_CAP[what]
                assert v.caps[cap] == good.caps[cap] - 1 and {k: x for k, x in v.caps.items() if k != cap} == {k: x for k, x in good.caps.items() if k != cap}
            assert S.summary_of(v, plan=True)["error"] == (S.E_CAPACITY if what in S.PLAN_SHORT else 0), v
            assert all(len(x) == 0 for x in S.want(v)[:-1] if x is not None), v
            for k in RIGHT_WHEN_SHORT.get((call, what), ("nal_count", "nal_found", "stream_bytes")):
                assert s[k] == S.summary_of(good)[k], (v, k)
    assert set(S.SHORT_CAP[w] for w in S.SHORTS[call] if w != "short_span") == set(S.case(call, "small").caps), "a variant a capacity"


@pytest.mark.parametrize("call", S.CALLS2)
def test_roomy_rtp_and_mp4_variants_give_the_exact_result(call):
    for which in S.SIZES:
        good = S.case(call, which)
        v = S.variant(good, "roomy")
        assert S.summary_of(v) == S.summary_of(good) and S.summary_of(v, plan=True) == S.summary_of(good, plan=True)
        for x, y in zip(S.want(v)[:-1], S.want(good)[:-1]):
            assert np.array_equal(x, y), v
        for cap, n in v.caps.items():
            assert n - good.caps[cap] in (S.ROOM_ITEMS, S.ROOM_BYTES), (v, cap)
            assert n - good.caps[cap] == (S.ROOM_BYTES if cap == "out_cap" and call != "rtpo" else S.ROOM_ITEMS), (v, cap)
        assert v.spare and all(v.room[k] == good.room[k] + v.spare.get(k, 0) for k in good.room)
        if call == "rtpo":
            assert v.a["prm"]["max_span"] > 2 * S.case(call, "large").a["prm"]["max_span"]
    assert S.ROOM_ITEMS == 3 * 256 + 1 and S.ROOM_BYTES == (64 << 10) + 1


def test_the_rtp_and_mp4_sequence_is_the_ten_steps_and_the_new_axis():
    for call in S.CALLS2:
        steps = S.sequence2(call)
        shorts = [("large " + w.replace("_", " "), False) for w in S.SHORTS[call]]
        assert [(c.name, plan) for c, plan in steps] == [("large", False), ("large roomy", False), ("small", False), ("large bad-late", False),
                                                          ("small", False), ("small bad-early", False), ("odd", False), ("empty", False)] + shorts + [
                                                              ("small roomy", False), ("large", True), ("large", False)]
        assert steps[0][0] is steps[-1][0] is steps[-2][0] is S.case(call, "large") and steps[2][0] is steps[4][0]


def test_the_pipelines_give_back_what_went_in():
    for which in ("small", "large"):
        for call in ("rtp", "rtpa"):
            pack = S.case(call, which)
            order = S.order_of(pack)
            unpack = S.unpack_of(order)
            assert order is S.order_of(pack) and unpack is S.unpack_of(order)
            s = S.summary_of(order)
            assert s["error"] == 0 and s["nal_count"] == S.summary_of(pack)["nal_count"] and s["reserved"][2] > 0 and s["reserved"][1] == 0
            assert not np.array_equal(order.a["off"], np.sort(order.a["off"])) and np.array_equal(S.want(order)[0], np.sort(order.a["off"]))
            a = pack.a
            nals = [a["stream"][int(x):int(y)].tobytes() for x, y in zip(a["index"]["start"], a["index"]["end"])]
            out, _, nal_au, _, s = S.want(unpack)
            assert s["error"] == 0 and s["reserved"][2] == 0 and out.tobytes() == b"".join(b"\x00\x00\x00\x01" + x for x in nals)
            assert np.array_equal(nal_au, a["nal_au"] - a["nal_au"][0])
        frag = S.case("mp4f", which)
        back = S.samples_of(frag)
        assert all(np.array_equal(S.want(back)[k], S.want(frag)[j]) for k, j in ((0, 1), (1, 2), (5, 3)))
        write = S.case("stblw", which)
        back = S.stbl_of(write)
        t = write.a["t"]
        assert S.want(back)[0].tolist() == t["off"] and S.want(back)[1].tolist() == t["size"]
        assert S.want(back)[2].tolist() == [x - t["dts"][0] for x in t["dts"]]
    assert S.plan_blocks(S.order_of(S.case("rtp", "large")))[0] >= 3 and S.plan_blocks(S.samples_of(S.case("mp4f", "large")))[1] >= 3
