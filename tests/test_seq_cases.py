"""The cases of tests/test_gpu_sequences.py are what that file takes them for, by the plain reference loops alone: the plan
workgroups each one fills, no error in the good ones, HBS_E_ARG with the edited entry named in the malformed ones, HBS_E_CAPACITY
in the ones a byte short.  The same for the RTP and MP4 calls of tests/test_gpu_sequences_rtp_mp4.py (S.CALLS2), with the output
tiles, a variant for each capacity that is one short, the roomy variants and the pipelines' later stages; and for the timing and
encryption calls of tests/test_gpu_sequences_times_crypt.py (S.CALLS3), with the spans of every AU table by the reference's
`spans` alone, the long clear runs and the workgroup edges of the subsample cases, the long entries in every range of the large
crypt tables, and the two cbcs references held against each other.  No GPU."""
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


# ---- the timing and encryption calls (S.CALLS3) -----------------------------------------------------------------------------------

@pytest.mark.parametrize("call", S.CALLS3)
def test_plan_workgroups_of_every_timing_and_crypt_case(call):
    small, large, odd = (S.case(call, w) for w in S.SIZES)
    assert all(b == 1 for b in S.plan_blocks(small)), (small, S.items(small))
    for n, per in S.items(large):
        assert S.blocks(n, per) >= 3 and n % per, (large, n, per)
    for lo, mid, hi in zip(S.plan_blocks(small), S.plan_blocks(odd), S.plan_blocks(large)):
        assert lo < mid < hi, (odd, S.items(odd), S.items(large))
    assert all(n == 0 for n, _ in S.items(S.empty(call)))
    if call == "aut":
        assert len(small.a["au"]) < S.AUT_BLOCK and len(large.a["au"]) >= 3 * S.AUT_BLOCK + 11
    elif call == "csub":
        assert len(large.a["index"]) >= 2 * S.CENC_NAL_BLOCK + 900 and 100 < len(small.a["index"]) < 1000
    else:
        assert len(small.a["off"]) < S.CRYPT_SAMPLE_BLOCK and S.crypt_entries(small.a) < S.CRYPT_RANGES
        assert len(large.a["off"]) >= 3 * S.CRYPT_SAMPLE_BLOCK + 40 and S.crypt_entries(large.a) >= 16 * S.CRYPT_RANGES + 300
        assert 8_000_000 < len(large.a["data"]) < 11_000_000


@pytest.mark.parametrize("call", S.CALLS3)
def test_good_timing_and_crypt_cases_and_the_empty_one_have_no_error(call):
    cases = [S.case(call, w) for w in S.SIZES] + [S.empty(call)] + ([S.hollow(call)] if call in S.CRYPT_CALLS else [])
    for c in cases:
        for plan in (True, False) if call in ("aut", "csub") else (False,):
            s = S.summary_of(c, plan)
            assert s["error"] == 0 and s["stop_reason"] == 0 and (call == "aut" or s["reserved"][0] == 0), (c, plan, s)
        out = S.want(c)[:-1]
        for name, x in zip((n for n, _ in S.AUT_TABLES) if call == "aut" else c.room, out):
            if name in c.room:                         # (hbs_au_times: the tables the case asks for)
                assert np.ascontiguousarray(x).view(np.uint8).size == c.room[name], (c, name)
    s = S.summary_of(S.empty(call))
    assert s["nal_count"] == 0 and s["nal_found"] == 0 and s["rbsp_bytes"] == 0 and s["reserved"][1:] == [0, 0], s
    if call in ("aut", "csub"):                    # a plan writes the summary, and hbs_cenc_subsamples' d_sub_first with it
        w = S.want(S.case(call, "large"), plan=True)
        assert [x is not None for x in w[:-1]] == ([False] * 4 if call == "aut" else [True, False])


@pytest.mark.parametrize("call", S.CALLS3)
def test_malformed_timing_and_crypt_variants_name_their_entry(call):
    """the summary word the header promises: reserved[0] = 1 + the AU, the NAL, the sample"""
    for which in ("small", "large"):
        good = S.case(call, which)
        for k, what in enumerate(("bad_early", "bad_late")):
            v = S.variant(good, what)
            n, per = v.among
            s = S.summary_of(v)
            assert v.named == (0, v.bad + 1) and s["error"] == v.error == (S.E_DEPTH if call == "aut" else S.E_ARG) and s["reserved"][0] == v.bad + 1, (v, s)
            if what == "bad_early":
                assert 0 <= v.bad < min(per, n), (v, v.bad)
            elif call == "aut":                    # the AU behind, whose backward walk offends, lies in the last workgroup
                assert (S.blocks(n, per) - 1) * per <= v.bad + S.T.MAX_SPAN + 1 < n, (v, v.bad)
            else:
                assert (S.blocks(n, per) - 1) * per <= v.bad < n, (v, v.bad, v.among)
            if call == "aut":                      # a span of the limit plus one, by the reference's spans alone; no table written
                back, fwd = S.T.spans(v.a["au"])
                assert max(int(back.max()), int(fwd.max())) == S.T.MAX_SPAN + 1 and int(fwd[v.bad]) == S.T.MAX_SPAN + 1
                assert np.flatnonzero((back > S.T.MAX_SPAN) | (fwd > S.T.MAX_SPAN)).tolist() == [v.bad, v.bad + S.T.MAX_SPAN + 1]
                assert all(x is None for x in S.want(v)[:-1]) and s["nal_count"] == 0 and s["reserved"][1:] == [0, 0]
                assert S.summary_of(v, plan=True) == s
            elif call == "csub":
                assert S.want(v)[0] is None and S.want(v)[1] is None and S.summary_of(v, plan=True)["error"] == S.E_ARG
                assert int(v.a["po"][v.bad]) == int(v.a["index"]["start"][v.bad]) + 1 and (v.a["keep"] is None or v.a["keep"][v.bad])
            else:                                  # counts 0, the data unchanged, and the check group the variant stands for
                assert s["nal_count"] == 0 and s["rbsp_bytes"] == 0 and S.want(v)[0] is v.a["data"]
                a, g = v.a, good.a
                fault = S.CRYPT_FAULTS[call][k]
                if fault == "sums":
                    assert int(a["size"][v.bad]) == int(g["size"][v.bad]) + 1 and int(a["off"][v.bad] + a["size"][v.bad]) <= int(a["off"][v.bad + 1])
                elif fault == "falling":
                    assert int(a["first"][v.bad + 1]) < int(a["first"][v.bad])
                else:
                    assert int(a["sub"]["clear"][int(a["first"][v.bad])]) == 65536
    if call in S.CRYPT_CALLS:                      # one fault of each check group over the variants of the three calls
        assert sorted(f for c in S.CRYPT_CALLS for f in S.CRYPT_FAULTS[c]) == sorted(["sums", "falling", "clear"] * 2)
        assert all({S.CRYPT_FAULTS[c][k] for c in S.CRYPT_CALLS} == {"sums", "falling", "clear"} for k in (0, 1))


def test_the_odd_timing_and_crypt_cases_differ():
    small, large, odd = (S.case("aut", w).a for w in S.SIZES)
    assert odd["kw"]["flags"] == S.T.WRAP33 and odd["outs"] == ("pts", "display") and len(small["outs"]) == len(large["outs"]) == 4
    s = S.summary_of(S.case("aut", "odd"))
    assert 0 < odd["kw"]["delay"] == s["reserved"][0] < s["reserved"][1] and s["reserved"][2] > 0          # a delay below R: late AUs
    w = S.want(S.case("aut", "odd"))
    assert int(w[1].max()) < 1 << 33 and int(w[1].min()) < 3003 * 400 and odd["kw"]["base_time"] < 1 << 33 < odd["kw"]["base_time"] + 3003 * 300
    small, large, odd = (S.case("csub", w).a for w in S.SIZES)
    assert odd["L"] == 1 and odd["keep"] is None and odd["po"] is None and odd["flags"] == S.CR.ALIGN16 and odd["clear_lead"] == 2
    assert small["L"] == large["L"] == 4 and all(x[k] is not None for x in (small, large) for k in ("keep", "po")) and small["flags"] == large["flags"] == 0
    assert (S.want(S.case("csub", "odd"))[1]["protect"] % 16 == 0).all()
    for call in S.CRYPT_CALLS:
        small, large, odd, hollow = [S.case(call, w).a for w in S.SIZES] + [S.hollow(call).a]
        per = np.diff(odd["first"].astype(np.int64))
        assert (per == 0).sum() > 100 and (per > 0).sum() > 100 and per[0] == 0 and per[-1] == 0 and (odd["size"][per == 0] == 0).all()
        assert (np.diff(odd["off"].astype(np.int64)) > 0).all() and (np.diff(small["first"].astype(np.int64)) > 0).all()
        assert not hollow["first"].any() and not hollow["size"].any() and len(hollow["sub"]) == 0 and len(hollow["off"]) > S.CRYPT_SAMPLE_BLOCK
        for a in (small, large):                   # odd addresses, gaps between the samples
            assert (a["off"] % 2 == 1).any() and (a["off"] % 16 != 0).any()
            assert (a["off"][1:].astype(np.int64) - (a["off"] + a["size"])[:-1].astype(np.int64) >= 1).all()
        if call == "cenc":
            assert odd["iv0"] is not None and odd["ivo"] and odd["iv"] is None and hollow["ivo"] and small["iv"] is not None and not small["ivo"]
            assert S.want(S.case(call, "odd"))[1][32:48].tolist() == [0] * 16          # the third counter block wrapped
        else:
            assert (odd["c"], odd["k"], odd["whole"]) == (3, 7, True) and odd["iv0"] is not None and odd["iv"] is None
            assert (small["c"], small["k"], large["c"], large["k"]) == (1, 9, 1, 0) and not small["whole"] and not large["whole"]


def test_every_au_times_table_is_inside_the_span_limit_by_the_reference():
    B, H = S.AUT_BLOCK, S.AUT_HALO
    for which in S.SIZES:
        back, fwd = S.T.spans(S.case("aut", which).a["au"])
        assert max(int(back.max()), int(fwd.max())) <= S.T.MAX_SPAN, which
    large = S.case("aut", "large").a["au"]
    back, fwd = S.T.spans(large)
    heads = S.T.heads_of(large)
    assert heads == [0, B - 1, B]                  # the last AU of a workgroup and the first of the next
    nopic = np.flatnonzero(large["flags"] & S.T.NO_PICTURE)
    assert nopic.min() < 2 * B <= nopic.max() and (np.diff(nopic) == 1).all()          # a run without a picture across a workgroup's edge
    assert H < int(fwd[3 * B - 1]) <= 100 and H < int(back[4 * B]) <= 100          # walks that leave the halo, both ways
    assert (3 * B - 1) % B == B - 1 and (4 * B) % B == 0


def test_the_large_subsample_case_crosses_both_workgroup_edges():
    large = S.case("csub", "large")
    a, (first, sub, s) = large.a, S.want(large)
    per = np.diff(first.astype(np.int64))
    assert (sub["clear"] == 65535).sum() >= 3 and s["reserved"][2] < len(a["index"])          # long clear runs; a d_keep that drops NALs
    alone = int(a["nal_au"][200] - a["nal_au"][0])
    assert sub[int(first[alone]):int(first[alone + 1])].tolist() == [(65535, 0), (65535, 0)]          # a clear run of exactly 2 x 65535
    above = int(a["nal_au"][50] - a["nal_au"][0])
    e = sub[int(first[above]):int(first[above + 1])]
    assert e[0].tolist() == (65535, 0) and 0 < e[1]["clear"] < 65535 and e[1]["protect"] > 0          # ... and one above 65535
    assert (per == 0).sum() >= 2                   # AUs with nothing kept
    for edge in (S.CENC_NAL_BLOCK, 2 * S.CENC_NAL_BLOCK):          # one AU and one clear run on both sides of the edge
        assert a["nal_au"][edge - 2] == a["nal_au"][edge + 1] and a["keep"][edge - 2:edge + 2].all()
        assert (((a["stream"][a["index"]["start"][edge - 2:edge + 2].astype(np.int64)] >> 1) & 63) >= 32).all()
    v = S.variant(large, "short")
    assert S.summary_of(v)["error"] == S.E_CAPACITY and v.caps["sub_cap"] == large.caps["sub_cap"] - 1 == s["nal_count"] - 1
    assert {k: x for k, x in S.summary_of(v).items() if k != "error"} == {k: x for k, x in s.items() if k != "error"}          # the counts are right
    assert S.want(v)[0] is None and S.want(v)[1] is None and S.summary_of(v, plan=True)["error"] == 0
    for which in S.SIZES:
        good = S.case("csub", which)
        r = S.variant(good, "roomy")
        assert S.summary_of(r) == S.summary_of(good) and r.caps["sub_cap"] == good.caps["sub_cap"] + S.ROOM_ITEMS
        assert r.room["sub"] == good.room["sub"] + 8 * S.ROOM_ITEMS == good.room["sub"] + r.spare["sub"] and r.room["sf"] == good.room["sf"]
        assert np.array_equal(S.want(r)[1], S.want(good)[1])


def test_the_large_crypt_tables_list_many_long_entries_in_every_range():
    a = S.case("cbcsd", "large").a
    listed, entries = S.long_entries_a_range(a)
    assert (listed > 4).sum() >= 900 and entries.min() >= 1 and entries.max() <= 256 and S.crypt_entries(a) % S.CRYPT_RANGES
    assert listed.min() >= 1 and listed.max() > 8          # more than two turns of the four wavefronts somewhere
    long_ = a["sub"]["protect"] // 16 >= S.CBCS_LANE_BLOCKS
    assert 0.45 < long_.mean() < 0.55 and int(a["sub"]["protect"][long_].max()) // 16 <= 70 and int(a["sub"]["protect"][~long_].max()) <= 48
    for call in ("cbcs", "cbcsd"):                 # 1:0: a long entry is kCbcsLaneBlocks crypt blocks and more
        c = S.case(call, "large").a
        assert S.CB.crypt_blocks(c["c"], c["k"], c["whole"], S.CBCS_LANE_BLOCKS) == S.CBCS_LANE_BLOCKS and c["sub"] is a["sub"]
    assert S.case("cenc", "large").a["data"] is a["data"]          # one set of tables a size


def test_the_sequential_and_the_batched_cbcs_reference_agree_on_the_small_cases():
    for call in ("cbcs", "cbcsd"):
        for c in (S.case(call, "small"), S.case(call, "odd"), S.hollow(call)):
            a = c.a
            out, done = S.CB.crypt(a["data"], a["off"], a["size"], a["first"], a["sub"], a["key"], iv=a["iv"], iv0=a["iv0"], c=a["c"], k=a["k"],
                                   whole=a["whole"], decrypt=call == "cbcsd")
            assert done == S.summary_of(c)["rbsp_bytes"] and np.array_equal(out, S.want(c)[0]), c
            assert (done > 0) == (c.name != "hollow") and (c.name == "hollow" or not np.array_equal(out, a["data"]))


def test_the_timing_and_crypt_sequences_are_the_stated_steps():
    for call in S.CALLS3:
        names = [(c.name, plan) for c, plan in S.sequence3(call)]
        want = [("large", False), ("small", False), ("large bad-late", False), ("small", False), ("small bad-early", False), ("odd", False)]
        want += [("hollow", False)] if call in S.CRYPT_CALLS else []
        want += [("empty", False)]
        want += [("large short", False), ("small roomy", False)] if call == "csub" else []
        want += [("large", True)] if call in ("aut", "csub") else []
        assert names == want + [("large", False)], call
    steps = S.shared_crypt_steps()
    assert [(c.call, c.name) for c, _ in steps] == list(S.SHARED_CRYPT) and steps[0][0] is S.case("cenc", "large")
    assert [c.call for c, _ in steps[:5]] == ["cenc", "cbcsd", "cbcs", "cenc", "cbcsd"] and S.summary_of(steps[7][0])["error"] == S.E_ARG
    assert S.summary_of(steps[8][0])["error"] == 0 and steps[5][0] is S.hollow("cenc")
