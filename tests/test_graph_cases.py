"""The families of tests/test_gpu_graphs.py are what the replays of a captured call need, by the reference loops alone: the
siblings of a family agree in every argument the host passes, no two of them give the same answer, each family has the members it
is meant to have and each member takes the path it is meant to take, and no sibling is left out of a replay list.  No GPU."""
import numpy as np
import pytest

from tests import _graph_cases as G
from tests import _seq_cases as S

IDS = [G.family_id(p) for p in G.FAMILIES]


def families(calls):
    return [p for p in G.FAMILIES if p[0].split(" ")[0] in calls]


def ids(ps):
    return [G.family_id(p) for p in ps]


def answer(c):
    """the reference's answer as bytes and numbers that compare"""
    w = G.want(c)
    if c.call == "parse":
        return tuple((e["rc"], tuple(e["nal"]), e["struct"].tobytes() if "struct" in e else b"") for e in w[0])
    s = w[-1]
    return tuple(b"" if x is None else G.as_bytes(x).tobytes() for x in w[:-1]) + (tuple(sorted((k, str(v)) for k, v in s.items())),)


@pytest.mark.parametrize("p", G.FAMILIES, ids=IDS)
def test_siblings_agree_in_every_host_argument(p):
    fam = G.family(*p)
    assert len(fam.members) >= 4, fam
    first = G.host_args(fam.members[fam.first()])
    for k, c in fam.members.items():
        assert c.call == fam.call and G.host_args(c) == first, (fam, k)
        for name in G.INPUTS[fam.call]:                    # a replay copies whole buffers
            assert G.as_bytes(c.a[name]).size == G.as_bytes(fam.members[fam.first()].a[name]).size, (fam, k, name)


@pytest.mark.parametrize("p", G.FAMILIES, ids=IDS)
def test_no_two_siblings_give_the_same_answer(p):
    fam = G.family(*p)
    seen = {}
    for k, c in fam.members.items():
        a = answer(c)
        for other, b in seen.items():
            assert a != b, (fam, k, other)
        seen[k] = a
    if fam.call not in ("parse", "keep", "ext"):           # the output bytes too, but for one pair that differs in a table alone (the way back
        outs = {seen[k][0] for k in fam.good()}            # from length prefixes: one stream under two sample tables)
        assert len(outs) >= len(fam.good()) - (1 if fam.call == "l2a" else 0), fam
    inputs = [tuple(G.as_bytes(c.a[n]).tobytes() for n in G.INPUTS[fam.call]) for c in fam.members.values()]
    assert len(set(inputs)) == len(inputs), fam


@pytest.mark.parametrize("p", G.FAMILIES, ids=IDS)
def test_errors_are_the_expected_ones_and_capacities_the_largest_need(p):
    fam = G.family(*p)
    if fam.call in ("parse", "keep", "ext"):
        return
    full = {key: False for key in fam.members[fam.first()].caps}
    for k, c in fam.members.items():
        s = G.summary_of(c)
        assert s["error"] == fam.errors.get(k, 0), (fam, k, s)
        if k in fam.errors:
            assert all(len(x) == 0 for x in G.want(c)[:-1] if x is not None), (fam, k)
            if fam.call in S.CALLS:
                assert S.reserved0(s) == (c.bad + 1 if S.names_the_entry(fam.call) else 0), (fam, k, s)
            continue
        need, _ = G.needs(c)
        for key, v in need.items():
            assert v <= c.caps[key], (fam, k, key)
            full[key] = full[key] or v == c.caps[key]
    assert all(full.values()), (fam, full)                   # some sibling fills each capacity to the last byte or entry


@pytest.mark.parametrize("p", G.FAMILIES, ids=IDS)
def test_no_sibling_is_left_out_of_a_replay_list(p):
    fam = G.family(*p)
    r = fam.replays()
    assert set(r) == set(fam.members) and r[-1] == fam.first() and r[0] != fam.first(), (fam, r)
    for j, k in enumerate(r[:-1]):
        if k in fam.errors:
            assert r[j + 1] not in fam.errors, (fam, r)    # an erroneous sibling directly in front of a good one
    assert all(k in r for k in fam.errors) and len(fam.good()) >= 3


def test_families_are_built_once():
    assert G.family("tsd", 192) is G.family("tsd", 192) and G.family("tsd", 192) is not G.family("tsd", 204)
    c = G.family("emit tiny").members["stretch"]
    assert G.want(c) is G.want(c)


# ---- the members and their paths ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", families(("a2l", "l2a", "flt")), ids=ids(families(("a2l", "l2a", "flt"))))
def test_piece_table_families(p):
    fam = G.family(*p)
    call, which = p[0].split(" ")
    first = fam.members[fam.first()]
    n = S.items(first)[0][0] if call != "flt" else len(first.a["idx"])
    per = S.SAMPLE_BLOCK if call == "l2a" else S.NAL_BLOCK
    assert (S.blocks(n, per) == 1) if which == "small" else (S.blocks(n, per) >= 3 and n % per), (fam, n)
    if call == "a2l":
        assert list(fam.members) == ["base", "mask", "index", "aus", "bad"]
        m = fam.members
        assert np.array_equal(m["base"].a["idx"], m["mask"].a["idx"]) and not np.array_equal(m["base"].a["keep"], m["mask"].a["keep"])
        assert not np.array_equal(m["base"].a["idx"], m["index"].a["idx"])
        assert not np.array_equal(m["base"].a["nal_au"], m["aus"].a["nal_au"]) and int(m["aus"].a["nal_au"][-1]) + 1 == first.a["n_aus"]
        assert all(c.a["keep"] is not None for c in m.values())
        assert not S.F.consistent(m["bad"].a["idx"], len(m["bad"].a["s"]))
    elif call == "l2a":
        assert list(fam.members) == ["base", "index", "aus", "short"]
        fw = G.family("a2l " + which).members[fam.first()]
        assert len(first.a["off"]) == fw.a["n_aus"]
        assert S.reserved0(G.summary_of(fam.members["short"])) == fam.members["short"].bad + 1
        for k in fam.good():                               # everything kept: the payloads of the forward sibling's whole index
            assert G.summary_of(fam.members[k])["nal_count"] == len(fw.a["idx"])
    else:
        assert list(fam.members) == ["rule 0", "rule 1", "rule 2", "mask", "index", "bad"]
        kept = [int(np.count_nonzero(fam.members["rule %d" % k].a["keep"])) for k in range(3)]
        assert kept[0] == n and 0 < kept[1] < n and 0 < kept[2] < n and kept[1] != kept[2], kept
        assert not S.F.consistent(fam.members["bad"].a["idx"], len(first.a["s"]))
        assert fam.members["bad"].bad >= (S.blocks(n, per) - 1) * per
    for c in fam.members.values():
        assert 0 < c.caps["out_cap"] < (4 << 20)


@pytest.mark.parametrize("p", families(("tsd", "tsm")), ids=ids(families(("tsd", "tsm"))))
def test_transport_families(p):
    fam = G.family(*p)
    first = fam.members[fam.first()]
    assert S.plan_blocks(first)[0] == 2 and S.items(first)[0][0] % S.items(first)[0][1]
    if p[0] == "tsd":
        assert list(fam.members) == ["most", "few", "all", "late", "fault"] and first.a["B"] == p[1]
        firsts = {k: int(G.want(fam.members[k])[1]["packet"][0]) for k in fam.good()}       # the first PES start falls elsewhere in each
        assert len(set(firsts.values())) == len(firsts), firsts
        assert fam.members["fault"].bad >= S.PACKET_BLOCK                                  # in the second plan workgroup
    else:
        assert list(fam.members) == ["one", "two", "three", "pts", "begin"] and first.a["prm"]["packet_bytes"] == p[1]
        assert int(fam.members["pts"].a["pts"][fam.members["pts"].bad]) == 1 << 33
        au, at = fam.members["begin"].a["au"], fam.members["begin"].bad
        assert int(au["unit_begin"][at]) > int(au["unit_end"][at])
        assert fam.members["pts"].bad >= S.TSM_AU_BLOCK > fam.members["begin"].bad
        lens = {len(S.want(c, plan=True)[0]) for c in (fam.members[k] for k in fam.good())}
        assert len(lens) >= 2                              # other output sizes under one capacity


def test_au_insert_family():
    fam = G.family("ins")
    assert list(fam.members) == ["six", "three", "ten", "sets", "tables"]
    first = fam.members["six"]
    (nals, per_n), (aus, per_a) = S.items(first)
    assert S.blocks(aus, per_a) == 2 and aus % per_a and nals > aus
    irap, auds, sets = {}, {}, {}
    for k in fam.good():
        c = fam.members[k]
        s = G.summary_of(c)
        irap[k] = tuple(np.flatnonzero(c.a["au"]["flags"] & 1)[:8])
        auds[k], sets[k] = s["reserved"][0], s["reserved"][1]
        assert s["reserved"][2] == aus and s["reserved"][0] > 0 and s["reserved"][1] > 0, (k, s)
    assert len(set(irap.values())) == 4 and len(set(auds.values())) == 4 and len(set(sets.values())) >= 3, (irap, auds, sets)
    bad = fam.members["tables"]
    assert int(bad.a["au"]["nal_count"][bad.bad]) == int(first.a["au"]["nal_count"][bad.bad]) + 1


def test_au_keep_family():
    fam = G.family("keep")
    assert list(fam.members) == ["one", "two", "three", "no sets"] and not fam.errors
    for k, c in fam.members.items():
        a, keep = c.a, G.want(c)[0]
        assert len(a["nal_au"]) == G.KEEP_NALS > 4 * 256 and G.KEEP_NALS % 256 and int(a["nal_au"][-1]) + 1 == G.KEEP_AUS
        inside = (a["nal_au"] >= a["first"]) & (a["nal_au"] < a["first"] + a["count"])
        assert 0 < inside.sum() < G.KEEP_NALS and np.all(keep[inside] == 1)
        extra = np.flatnonzero((keep == 1) & ~inside)
        assert len(extra) == (0 if k == "no sets" else 3), (k, extra)      # the VPS, the SPS and the PPS in force
        assert all(int(a["parsed"]["rc"][x]) >= 0 and int(a["nal_au"][x]) < a["first"] for x in extra)
    firsts = {int(np.flatnonzero(c.a["nal_au"] >= c.a["first"])[0]) for c in fam.members.values()}
    assert len(firsts) == 4                                # the range begins at another NAL in each


def test_parse_extended_family():
    from tests.test_ext_types import as_tuple
    fam = G.family("ext")
    assert list(fam.members) == ["one", "two", "three", "four"] and not fam.errors
    assert G.EXT_NALS > 2 * 256 and G.EXT_NALS % 256
    for k, c in fam.members.items():
        rcs, recs = G.want(c)[:2]
        types = [(nal[0] >> 1) & 63 for nal in c.a["nals"]]
        assert set(range(35, 41)) <= set(types) and any(t < 35 for t in types), (k, sorted(set(types)))
        extended = rcs != G.NOT_EXTENDED
        assert extended.sum() > 400 and (~extended).sum() > 20, (k, int(extended.sum()))
        assert all(35 <= types[i] <= 40 for i in np.flatnonzero(extended))
        assert not G.as_bytes(recs[~extended]).any()                                  # zeroed records for the others
        assert (rcs[extended] == -1).any() and (rcs[extended] > 0).any(), k           # cursors past the RBSP and NALs read through
        assert any(as_tuple(int(rcs[i]), recs[i])[3] > 1 for i in np.flatnonzero(extended)), k      # an SEI NAL of several messages


def dense_tiles(arena):
    """tiles of the arena with a stretch of 16 KiB and more that is all zero pairs in front of a byte <= 3"""
    a = arena.astype(np.int16)
    hit = (a[:-2] == 0) & (a[1:-1] == 0) & (a[2:] <= 3)
    out = []
    for t in range(len(arena) // G.T + 1):
        if np.count_nonzero(hit[t * G.T:(t + 1) * G.T]) >= 16384 // 3:
            out.append(t)
    return out


def test_emit_families():
    pin = G.family("emit pinned")
    assert list(pin.members) == ["tile 3", "gone", "tiles 6-7", "zeros", "plain"] and not pin.errors
    first = pin.members["tile 3"]
    assert len(first.a["idx"]) == 40 and len(first.a["arena"]) // G.T >= 9
    assert all(np.array_equal(c.a["idx"], first.a["idx"]) for c in pin.members.values())          # one index for all
    assert [dense_tiles(pin.members[k].a["arena"]) for k in pin.members] == [[3], [], [6, 7], [7], []]
    moved = pin.members["tiles 6-7"].a["arena"]
    for tile in (2, 5):                                    # listed (a pattern in every sampled chunk), not dense
        assert all(tuple(moved[G.sample_at(tile, sec, sub) + 5: G.sample_at(tile, sec, sub) + 8]) == (0, 0, 1) for sec in range(12) for sub in range(4))
        assert all(G.sample_at(tile, sec, 3) + 8 <= (tile + 1) * G.T for sec in range(12))
    z = pin.members["zeros"].a["arena"]
    assert not z[7 * G.T + 70_000: 7 * G.T + 90_000].any()
    auto = G.family("emit auto")
    assert list(auto.members) == ["sparse", "zero-heavy", "holes", "sparse 2"] and not auto.errors
    n, total = len(auto.members["sparse"].a["idx"]), len(auto.members["sparse"].a["arena"])
    assert n <= G.EMIT_SMALL_NALS and total > (32 << 10) and total // n >= G.TINY_MEAN        # neither the one launch nor the tiny path
    share = {k: float(np.mean(c.a["arena"] == 0)) for k, c in auto.members.items()}
    assert share["zero-heavy"] > 0.1 and max(share["sparse"], share["holes"], share["sparse 2"]) < 0.01, share
    idx = auto.members["holes"].a["idx"]
    assert np.all(idx["rbsp_off"][1:] > idx["rbsp_off"][:-1] + idx["rbsp_len"][:-1])          # not back to back: no arena tiles
    tiny = G.family("emit tiny")
    assert list(tiny.members) == ["stretch", "zeros", "holes", "outside"]
    c = tiny.members["stretch"]
    n, total = len(c.a["idx"]), len(c.a["arena"])
    assert n > G.EMIT_SMALL_NALS and 48 <= total // n <= 80 and n % 64                         # the tiny path, a ragged last group
    idx = c.a["idx"]
    assert np.array_equal(idx["rbsp_off"][1:], idx["rbsp_off"][:-1] + idx["rbsp_len"][:-1])   # one stretch: groups of 64
    idx = tiny.members["holes"].a["idx"]
    assert np.any(idx["rbsp_off"][1:] > idx["rbsp_off"][:-1] + idx["rbsp_len"][:-1])
    bad = tiny.members["outside"]
    assert int(bad.a["idx"]["rbsp_off"][bad.bad]) > total and bad.bad >= n - 64                # in the last group


@pytest.mark.parametrize("name,n", [("parse large", G.PARSE_LARGE), ("parse few", G.PARSE_FEW)])
def test_parse_families(name, n):
    """the CPU single-stepper says which siblings raise the flag and how many slices the exact re-walk takes"""
    from tests._parsecmp import compare
    fam = G.family(name)
    assert list(fam.members) == ["ordinary", "out of spec", "forbidden", "broken sets"] and not fam.errors
    assert (n <= G.PARSE_SMALL) == (name == "parse few") and all(len(c.a["idx"]) == n for c in fam.members.values())
    walked = {}
    for k, c in fam.members.items():
        parsed, structs, stats = G.parse_sim(c)
        compare(parsed, structs, c.a["arena"], c.a["idx"], G.want(c)[0])
        walked[k] = (stats[0], stats[1])
        assert stats[2] == 0 and 0 < len(structs) <= c.caps["structs_cap"], (k, stats)
    assert max(G.parse_need(c) for c in fam.members.values()) == fam.members["ordinary"].caps["structs_cap"]
    assert walked["ordinary"] == (0, 0), walked
    assert walked["out of spec"][0] == 1 and walked["out of spec"][1] >= 2, walked
    assert walked["forbidden"][0] == 1, walked
    rcs = [e["rc"] for e in G.want(fam.members["broken sets"])[0] if e.get("kind") in ("vps", "sps", "pps")]
    assert any(rc < 0 for rc in rcs), rcs
