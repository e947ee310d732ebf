"""The inputs of tests/test_gpu_graphs.py: for each enqueue-only call a FAMILY of siblings that agree in every argument the host
passes (counts, byte sizes, capacities, flags, params) and differ only in what lies in device memory, so that one captured call
can be replayed on each of them in the same buffers.  The shorter inputs of a family are padded to the longest with bytes no
entry covers, the capacities are the largest of the siblings' needs.  numpy only, in the style of tests/_seq_cases.py, whose
builders, reference loops and constants are used again; tests/test_graph_cases.py holds on the CPU that the families are what the
replays need.

A sibling is a _seq_cases.Case (`a`: the call's arguments, `caps`, `room`, `bad`); want(case) is the reference's answer.  The
calls of _seq_cases.py keep their names (a2l, l2a, tsd, tsm, ins); "flt" is hbs_filter_annexb, "emit" hbs_emit_annexb and
"parse" hbs_parse_headers, whose answers come from the filter's plain loop and from the oracle, "keep" hbs_au_keep (tests/_au_ref.py),
"ext" hbs_parse_extended (the oracle's orc_read_extended_nal per NAL)."""
import numpy as np

from tests import _au_ref as AU
from tests import _auins_ref as INS
from tests import _filter_ref as F
from tests import _seq_cases as S
from tests import _ts_ref as TSD
from tests import _tsmux_ref as TSM
from tests._orc import NAL_ENTRY

E_ARG, E_CAPACITY = S.E_ARG, S.E_CAPACITY
PACKET_SIZES = (188, 192, 204)
T = 192 * 1024                                        # an arena tile of the emit kernel by tiles (hbs_emit.hip: kTTileBytes)
TINY_MEAN = 448                                       # below this mean the automatic emit takes its path for tiny NALs (kTinyMeanBytes)
EMIT_SMALL_NALS = 256                                 # up to here a handful of small NALs is one launch (kEmitSmallNals)
PARSE_SMALL = 64                                      # up to here hbs_parse_headers is the k4_small + k4_seq chain
# the device inputs of a call, by their names in Case.a: what a replay copies into the captured buffers
INPUTS = dict(a2l=("s", "idx", "keep", "nal_au"), l2a=("data", "off", "size"), tsd=("ts",), tsm=("stream", "au", "pts", "dts"),
              ins=("stream", "index", "parsed", "au", "nal_au"), flt=("s", "idx", "keep"), emit=("arena", "idx"), parse=("arena", "idx"),
              keep=("nal_au", "parsed"), ext=("arena", "idx"))
# the numbers the host passes next to them
SCALARS = dict(a2l=("L", "n_aus"), l2a=("L", "sc"), tsd=("B", "pid"), tsm=(), ins=("first", "count", "flags"), flt=(), emit=("gap_mode",), parse=(),
               keep=("first", "count", "param_sets"), ext=())


class Family:
    """members: {label: Case} in order, the first one is what is captured; errors: {label: the error its summary reports}"""

    def __init__(self, name, call, members, errors=()):
        self.name, self.call, self.members, self.errors = name, call, dict(members), dict(errors)

    def __repr__(self):
        return self.name

    def first(self):
        return next(iter(self.members))

    def good(self):
        return [k for k in self.members if k not in self.errors]

    def replays(self):
        """every sibling but the captured one, the captured one, every erroneous sibling directly in front of a good one, and the
        captured one at the end -> labels"""
        first, good = self.first(), self.good()
        out = [k for k in good if k != first] + [first]
        for j, k in enumerate(self.errors):
            out += [k, good[(j + 1) % len(good)]]
        if out[-1] != first:
            out.append(first)
        return out


def as_bytes(x):
    return np.ascontiguousarray(x).view(np.uint8).reshape(-1)


def host_args(case):
    """everything the host passes with the call: the byte size and item count of every input, the numbers, the capacities"""
    a = case.a
    sizes = tuple((k, len(a[k]), as_bytes(a[k]).size) for k in INPUTS[case.call])
    prm = tuple(sorted(a["prm"].items())) if case.call == "tsm" else ()
    return sizes, tuple((k, a[k]) for k in SCALARS[case.call]), prm, tuple(sorted(case.caps.items())), tuple(sorted(case.room.items()))


def padded(rng, x, n):
    """x with bytes behind it that no entry covers, n bytes in all"""
    assert len(x) <= n
    return np.concatenate([x, rng.integers(1, 256, size=n - len(x), dtype=np.uint8)])


def pad_input(rng, cases, name):
    n = max(len(c.a[name]) for c in cases)
    for c in cases:
        c.a[name] = padded(rng, c.a[name], n)


# ---- what the references say ---------------------------------------------------------------------------------------------------

def filter_reference(a, out_cap):
    """tests/_filter_ref.py with the two errors of the header: an inconsistent index (the sizes then mean nothing), an output
    that does not fit (the sizes are reported all the same); nothing is written either way"""
    none = (np.zeros(0, np.uint8), np.zeros(0, dtype=F.NAL_ENTRY))
    if not F.consistent(a["idx"], len(a["s"])):
        return none + (dict(error=E_ARG),)
    out, io, s = F.filter_ref(a["s"], a["idx"], a["keep"])
    if out_cap is not None and len(out) > out_cap:
        return none + (dict(s, error=E_CAPACITY),)
    return out, io, s


def emit_reference(a, out_cap):
    """the oracle's rbsp_to_nal per NAL behind its gap -> (out, index_out, summary) as hbs_emit.hip's summary kernels fill it"""
    from tests import _orc
    orc = _orc.oracle()
    arena, idx, n = a["arena"], a["idx"], len(a["idx"])
    s = dict(nal_count=n, nal_found=n, rbsp_bytes=len(arena), stream_bytes=0, stop_reason=-1 if n else 0, error=0)
    none = (np.zeros(0, np.uint8), np.zeros(0, dtype=NAL_ENTRY))
    if np.any(idx["rbsp_off"].astype(object) + idx["rbsp_len"].astype(object) > len(arena)):
        return none + ({k: v for k, v in dict(s, error=E_ARG).items() if k != "stream_bytes"},)      # (nothing was emitted: no size to report)
    out = orc.emit_annexb(arena, idx)
    io = np.zeros(n, dtype=NAL_ENTRY)
    pos = prev_end = 0
    for k in range(n):
        off, ln = int(idx["rbsp_off"][k]), int(idx["rbsp_len"][k])
        gap = (4 if k % 4 == 0 else 3) if a["gap_mode"] else max(int(idx["start"][k]) - prev_end, 0)
        prev_end = int(idx["end"][k])
        emitted = orc.rbsp_to_nal(arena[off:off + ln])[0]
        io[k] = (pos + gap, pos + gap + emitted, off, ln, 0)
        pos += gap + emitted
    assert pos == len(out), (pos, len(out))
    s["stream_bytes"] = len(out)
    if out_cap is not None and len(out) > out_cap:
        return none + (dict(s, error=E_CAPACITY),)
    return out, io, s


def reference(case, plan=False):
    c = {} if plan else case.caps
    if case.call == "flt":
        return filter_reference(case.a, c.get("out_cap"))
    if case.call == "emit":
        return emit_reference(case.a, c.get("out_cap"))
    if case.call == "parse":
        from tests._parsecmp import oracle_pass
        return (oracle_pass(case.a["nals"]),)
    if case.call == "ext":
        return ext_reference(case.a["nals"]) + (dict(error=0),)
    if case.call == "keep":                                # (no summary: the mask is all the call writes)
        a = case.a
        return AU.au_keep(a["nal_au"], a["parsed"], a["first"], a["count"], bool(a["param_sets"])), dict(error=0)
    return S.reference(case, plan)


def want(case, plan=False):
    """reference(), computed once: the tests share it and leave it unchanged"""
    if plan not in case._want:
        case._want[plan] = reference(case, plan)
    return case._want[plan]


def summary_of(case, plan=False):
    return want(case, plan)[-1]


def needs(case):
    if case.call == "flt":
        s = summary_of(case, plan=True)
        return dict(out_cap=s["stream_bytes"]), dict(out=s["stream_bytes"], io=s["nal_count"] * 32)
    if case.call == "emit":
        s = summary_of(case, plan=True)
        return dict(out_cap=s["stream_bytes"]), dict(out=s["stream_bytes"], io=s["nal_count"] * 32)
    if case.call == "parse":                               # the struct arena the CPU single-stepper plans (tests/_sim.py)
        need = parse_need(case)
        return dict(structs_cap=need), dict(structs=need, parsed=len(case.a["idx"]) * 32)
    if case.call == "keep":
        return {}, dict(keep=len(case.a["nal_au"]))
    if case.call == "ext":
        from tests.test_ext_types import EXT
        return {}, dict(parsed=len(case.a["idx"]) * 32, ext=len(case.a["idx"]) * EXT.itemsize)
    return S.needs(case)


def settle(family):
    """the capacities and the room of every sibling: the largest of what the good ones need"""
    caps, room = {}, {}
    for k in family.good():
        c, r = needs(family.members[k])
        for d, src in ((caps, c), (room, r)):
            for key, v in src.items():
                d[key] = max(d.get(key, 0), v)
    for c in family.members.values():
        assert not c._want.get(False), c                   # (the reference of a run looks at the capacities)
        c.caps, c.room = dict(caps), dict(room)
    return family


_families = {}


def family(name, B=188):
    """the family `name` (built once a process)"""
    key = (name, B if name in ("tsd", "tsm") else None)
    if key not in _families:
        _families[key] = settle(MAKERS[name](B) if name in ("tsd", "tsm") else MAKERS[name]())
    return _families[key]


# ---- the framing and transport calls -------------------------------------------------------------------------------------------

def au_cuts(rng, n, n_aus):
    """an AU numbering of n NALs with exactly n_aus AUs: n_aus - 1 cut points drawn at random"""
    step = np.zeros(n, dtype=np.uint32)
    step[rng.choice(np.arange(1, n), size=n_aus - 1, replace=False)] = 1
    return np.cumsum(step).astype(np.uint32)


def kept(rng, idx, p, L):
    return (rng.random(len(idx)) < p) & ((idx["end"] - idx["start"]) < (1 << (8 * L)))


def make_a2l(which):
    """another keep mask, another index of the same count, another AU numbering of the same n_aus, an inconsistent index"""
    p = S.A2L[which]
    rng = np.random.default_rng(300 + len(which))
    L = p["L"]
    s0, idx0 = S.indexed_stream(rng, p["nals"], p["mean"])
    s1, idx1 = S.indexed_stream(rng, p["nals"], p["mean"])
    nal_au, n_aus = S.au_numbers(rng, p["nals"], *p["aus"])

    def one(name, s, idx, keep_p, nal_au):
        return S.Case("a2l", "%s %s" % (which, name), dict(s=s, idx=idx, keep=kept(rng, idx, keep_p, L), L=L, nal_au=nal_au, n_aus=n_aus))
    m = dict(base=one("base", s0, idx0, 0.6, nal_au), mask=one("mask", s0, idx0, 0.3, nal_au), index=one("index", s1, idx1, 0.6, nal_au),
             aus=one("aus", s0, idx0, 0.6, au_cuts(rng, p["nals"], n_aus)))
    pad_input(rng, list(m.values()), "s")
    m["bad"] = S.malformed(m["base"], late=True)
    return Family("a2l " + which, "a2l", m, dict(bad=E_ARG))


def make_l2a(which):
    """the outputs of three forward siblings with everything kept, under one n_samples; one sample a byte short"""
    fw = family("a2l " + which).members
    rng = np.random.default_rng(310 + len(which))
    m = {}
    for name in ("base", "index", "aus"):
        a = fw[name].a
        out, _, so, s = S.LP.to_lenpref_ref(a["s"], a["idx"], None, a["L"], a["nal_au"], a["n_aus"])
        assert s["error"] == 0
        so = so.astype(np.int64)
        m[name] = S.Case("l2a", "%s %s" % (which, name), dict(data=out, off=so[:-1].astype(np.uint64), size=np.diff(so).astype(np.uint64), L=a["L"], sc=S.A2L[which]["sc"]))
    pad_input(rng, list(m.values()), "data")
    m["short"] = S.malformed(m["base"], late=True)
    return Family("l2a " + which, "l2a", m, dict(short=E_ARG))


TSD_PACKETS = S.PACKET_BLOCK + 300                    # two plan workgroups, the second one ragged


def make_tsd(B):
    """random_ts of one packet count with other seeds, shares of the PID, first PES starts and breaks; one of FAULTS"""
    m = {}
    for k, (name, kw) in enumerate((("most", dict(share=0.9, first_pes=2, p_break=0.02)), ("few", dict(share=0.4, first_pes=S.PACKET_BLOCK + 5, p_break=0.05, p_pes=0.15)),
                                    ("all", dict(share=1.0, first_pes=0, p_break=0.0)), ("late", dict(share=0.7, first_pes=700, p_break=0.1)))):
        ts = TSD.random_ts(np.random.default_rng(320 + 10 * k + B), TSD_PACKETS, B, S.PID, **kw)
        m[name] = S.Case("tsd", name, dict(ts=ts.reshape(-1), B=B, pid=S.PID))
    m["fault"] = S.malformed(m["most"], late=True)
    return Family("tsd %d" % B, "tsd", m, dict(fault=E_ARG))


TSM_AUS = S.TSM_AU_BLOCK + 100                        # two plan workgroups, the second one ragged


def make_tsm(B):
    """random_case of one AU count with other seeds; a PTS of 2^33; an AU whose unit_begin lies behind its unit_end"""
    prm = TSM.params(packet_bytes=B, flags=TSM.PCR, cc_es=5)
    rng = np.random.default_rng(340 + B)
    m = {}
    for name in ("one", "two", "three"):
        stream, au, pts, dts = TSM.random_case(rng, TSM_AUS, prm, max_es=300)
        m[name] = S.Case("tsm", name, dict(stream=stream, au=au, pts=pts, dts=dts, prm=prm))
    pad_input(rng, list(m.values()), "stream")
    m["pts"] = S.malformed(m["one"], late=True)
    m["begin"] = S.malformed(m["two"], late=False)
    return Family("tsm %d" % B, "tsm", m, dict(pts=E_ARG, begin=E_ARG))


INS_AUS = S.INS_AU_BLOCK + 44                         # two plan workgroups of the AU side, the second one ragged


def make_ins():
    """one count of NALs and of AUs: the shorter NAL lists end with further slice segments of their last picture; IRAP AUs, AUDs
    and the parameter sets in force fall elsewhere in each sibling; one sibling with inconsistent tables"""
    rng = np.random.default_rng(360)
    kinds = (("six", dict(irap_every=6)), ("three", dict(irap_every=3, max_slices=5, p_aud=0.5)), ("ten", dict(irap_every=10, p_aud=0.1, p_own_sets=0.5)),
             ("sets", dict(irap_every=4, p_own_sets=0.8, p_bad_set=0.1)))
    lists = {name: INS.random_aus(rng, INS_AUS, **kw) for name, kw in kinds}
    n = max(len(x) for x in lists.values())
    m = {}
    for name, nals in lists.items():
        last = [d for d in nals if d["type"] < 32 and d["layer"] == 0][-1]
        nals = nals + [dict(last, first=0, size=int(rng.integers(3, 60)), zeros=0, junk=0) for _ in range(n - len(nals))]
        stream, index, parsed, compact, au, nal_au = INS.build(rng, nals)
        assert len(index) == n and len(au) == INS_AUS, (name, len(index), len(au))
        m[name] = S.Case("ins", name, dict(stream=stream, index=index, parsed=parsed, compact=compact, au=au, nal_au=nal_au, first=0, count=INS_AUS, flags=7))
    pad_input(rng, list(m.values()), "stream")
    m["tables"] = S.malformed(m["six"], late=False)
    return Family("ins", "ins", m, dict(tables=E_ARG))


# ---- hbs_filter_annexb ---------------------------------------------------------------------------------------------------------

RULES = (dict(), dict(keep_types=((1 << 22) - (1 << 16)) | (7 << 32), max_temporal_id_plus1=7), dict(max_temporal_id_plus1=2, max_layer_id=0, keep_short=False))


def make_flt(which):
    """the streams of the length-prefix shapes.  The call is made with a keep mask: a rule is a record the HOST passes, so the
    siblings' rules differ in the masks that tests/_filter_ref.py's rule_keep makes of them; then a random mask, another index of
    the same count, and an inconsistent index"""
    p = S.A2L[which]
    rng = np.random.default_rng(380 + len(which))
    s0, idx0 = S.indexed_stream(rng, p["nals"], p["mean"])
    s1, idx1 = S.indexed_stream(rng, p["nals"], p["mean"])
    m = {"rule %d" % k: S.Case("flt", "%s rule %d" % (which, k), dict(s=s0, idx=idx0, keep=F.rule_keep(s0, idx0, **r))) for k, r in enumerate(RULES)}
    m["mask"] = S.Case("flt", which + " mask", dict(s=s0, idx=idx0, keep=rng.random(len(idx0)) < 0.5))
    m["index"] = S.Case("flt", which + " index", dict(s=s1, idx=idx1, keep=rng.random(len(idx1)) < 0.7))
    pad_input(rng, list(m.values()), "s")
    bad = dict(m["mask"].a, idx=m["mask"].a["idx"].copy())
    at = S.edited_entry(S.Case("a2l", "", dict(idx=idx0)), late=True)                # the edit of malformed() for an index
    bad["idx"]["start"][at] = bad["idx"]["end"][at - 1] - 1
    m["bad"] = S.Case("flt", which + " bad", bad, bad=at)
    return Family("flt " + which, "flt", m, dict(bad=E_ARG))


# ---- hbs_emit_annexb -----------------------------------------------------------------------------------------------------------

def stretch_index(lens, gaps, offs=None):
    """tests/test_gpu_emit.py's fake_index: NAL k of lens[k] RBSP bytes at offs[k] (default: back to back), gaps[k] bytes in front"""
    lens = np.asarray(lens, dtype=np.int64)
    idx = np.zeros(len(lens), dtype=NAL_ENTRY)
    idx["rbsp_off"] = np.concatenate([[0], np.cumsum(lens[:-1])]) if offs is None else offs
    idx["rbsp_len"] = lens
    end = np.cumsum(lens + np.asarray(gaps, dtype=np.int64))
    idx["end"], idx["start"] = end, end - lens
    return idx


def sample_at(tile, sec, sub):                        # hbs_emit.hip: k3t_sample
    return tile * T + 16384 * sec + 1024 * ((5 * sec + tile) & 15) + 64 * ((7 * sec + (tile >> 2)) & 15) + 16 * sub


def listed_not_dense(arena, tile):
    """a pattern in each of the 48 chunks the sample looks at, the rest of the tile clean"""
    for sec in range(12):
        for sub in range(4):
            x = sample_at(tile, sec, sub)
            arena[x + 5: x + 8] = (0, 0, 1)


def long_nals(seed=97):
    """tests/test_gpu_emit.py::test_emit_arena_tiles_count_dense_tiles_ahead: 40 NALs of 20-90 KB"""
    rng = np.random.RandomState(seed)
    lens = [int(x) for x in rng.randint(20000, 90000, size=40)]
    arena = rng.randint(1, 256, size=sum(lens)).astype(np.uint8)
    return rng, lens, arena, stretch_index(lens, [3 + (k & 1) for k in range(len(lens))])


def emit_case(name, arena, idx, gap_mode=0):
    return S.Case("emit", name, dict(arena=arena, idx=idx, gap_mode=gap_mode))


def make_emit_pinned():
    """the arena tiles pinned, dense tiles counted ahead; one index for all: a stretch of 00 00 03 in tile 3; the stretch gone; the
    stretch in tiles 6-7 with tiles 2 and 5 listed but not dense; 20 KiB of zeros between the sampled sectors; nothing dense"""
    rng, lens, base, idx = long_nals()
    assert len(base) // T >= 9
    pat = np.tile(np.array([0, 0, 3], dtype=np.uint8), 50_000)
    m = {}
    a = base.copy()
    a[3 * T + 1000: 3 * T + 1000 + 150_000] = pat
    m["tile 3"] = emit_case("tile 3", a, idx)
    a = base.copy()
    a[3 * T + 1000: 3 * T + 1000 + 150_000] = rng.randint(1, 256, size=150_000)
    m["gone"] = emit_case("gone", a, idx)
    a = base.copy()
    a[6 * T + 90_000: 6 * T + 90_000 + 150_000] = pat
    for tile in (2, 5):
        listed_not_dense(a, tile)
    m["tiles 6-7"] = emit_case("tiles 6-7", a, idx)
    a = base.copy()
    a[7 * T + 70_000: 7 * T + 90_000] = 0
    m["zeros"] = emit_case("zeros", a, idx)
    m["plain"] = emit_case("plain", base.copy(), idx)
    return Family("emit pinned", "emit", m)


def make_emit_auto():
    """the same NAL lengths on the automatic path: two sparse arenas, a zero-heavy one (12 % zeros: meant for count / scan / emit;
    the tests hold its bytes, not the chain the device's probe picks), and an
    index that is not one stretch of the arena.  (An arena of this size is below the 192 MiB from which the automatic path tries
    the arena tiles at all, so hbs_ctx_last_emit_by_tiles is 0 for every sibling: the kernel by NALs or the three steps run.)"""
    rng, lens, base, idx = long_nals(98)
    m = dict(sparse=emit_case("sparse", base, idx))
    a = base.copy()
    a[rng.rand(len(a)) < 0.12] = 0
    m["zero-heavy"] = emit_case("zero-heavy", a, idx)
    short = np.asarray(lens) - rng.randint(1, 40, size=len(lens))                  # bytes between the NALs that are nobody's
    m["holes"] = emit_case("holes", base, stretch_index(short, [3 + (k & 1) for k in range(len(lens))], offs=idx["rbsp_off"]))
    b = rng.randint(1, 256, size=len(base)).astype(np.uint8)
    for q in rng.randint(0, len(b) - 8, size=300):
        b[q:q + 3] = (0, 0, int(rng.randint(0, 4)))
    m["sparse 2"] = emit_case("sparse 2", b, idx)
    return Family("emit auto", "emit", m)


TINY_NALS = 64 * 40 + 21                              # forty wavefronts of the group kernel and a ragged one


def make_emit_tiny():
    """arenas of tiny NALs (a mean of 64 bytes, tests/test_gpu_emit.py::test_emit_tiny_nals_by_groups_of_64) on the automatic path:
    an index that is one stretch of the arena (groups of 64), the same with zero-heavy bytes (groups that take the exact walk), an
    index with holes in the arena (a lane per NAL), an entry outside rbsp_bytes (HBS_E_ARG)"""
    rng = np.random.RandomState(664)
    lens = [int(x) for x in rng.randint(0, 129, size=TINY_NALS)]
    lens[:8] = [0, 1, 2, 15, 16, 17, 0, 0]
    gaps = [int(rng.randint(3, 16)) for _ in lens]
    arena = rng.randint(0, 256, size=sum(lens)).astype(np.uint8)
    for q in rng.randint(0, len(arena) - 8, size=40):
        arena[q:q + 3] = (0, 0, int(rng.randint(0, 4)))
    idx = stretch_index(lens, gaps)
    m = dict(stretch=emit_case("stretch", arena, idx))
    z = arena.copy()
    z[rng.rand(len(z)) < 0.3] = 0
    m["zeros"] = emit_case("zeros", z, idx)
    short = np.maximum(np.asarray(lens) - rng.randint(0, 4, size=len(lens)), 0)
    m["holes"] = emit_case("holes", arena, stretch_index(short, gaps, offs=idx["rbsp_off"]))
    bad = idx.copy()
    bad["rbsp_off"][TINY_NALS - 7] = np.uint64(1 << 33)
    m["outside"] = emit_case("outside", arena, bad)
    m["outside"].bad = TINY_NALS - 7
    return Family("emit tiny", "emit", m, dict(outside=E_ARG))


# ---- hbs_parse_headers ---------------------------------------------------------------------------------------------------------

FORBIDDEN_SEEDS = (1036, 1064, 1320, 1496, 5224)      # tests/test_gpu_parse.py::test_default_batch_is_the_reference_on_forbidden_streams


def nal_lists(n):
    """-> {label: n NALs}: an ordinary stream, one with out-of-spec slices (walked again by k4_fix), the forbidden seeds, broken
    parameter sets"""
    from tests.hevc_synth import stream_4k30
    from tests.test_sim_parse_logic import broken, sequence
    from tests import _orc
    out = {}
    nals = []
    for seed in range(200, 200 + n // 13 + 1):
        nals += sequence(seed)
    out["ordinary"] = nals[:n]
    stream, _ = stream_4k30(21, n_pictures=n // 8 + 1, slices_per_picture=8, idr_every=60, payload_bytes=(60, 120), forbidden_every=7)
    s = np.frombuffer(stream, dtype=np.uint8)
    idx, _ = _orc.oracle().index_stream(s)
    out["out of spec"] = [bytes(s[int(a):int(b)]) for a, b in zip(idx["start"], idx["end"])][:n]
    nals = []
    for k in range(n // 13 + 1):
        seed = FORBIDDEN_SEEDS[k % len(FORBIDDEN_SEEDS)] if k % 2 == 0 or n <= PARSE_SMALL else 300 + k
        nals += broken(sequence(seed), np.random.RandomState(7 * seed + 2), lambda t: True) if seed > 1000 else sequence(seed)
    out["forbidden"] = nals[:n]
    nals = []
    for seed in range(6000, 6000 + n // 13 + 1):
        nals += broken(sequence(seed), np.random.RandomState(7 * seed + 2), lambda t: True)
    out["broken sets"] = nals[:n]
    return out


def parse_sim(case):
    """the batch single-stepped on the CPU with the re-walk the library makes -> (parsed, structs, [flag raised, slices walked again,
    chains too deep]), computed once"""
    if "sim" not in case._want:
        from tests import _sim
        idx, stats = case.a["idx"], []
        used = int(idx["rbsp_off"][-1]) + int(idx["rbsp_len"][-1])
        parsed, structs = _sim.parse_headers(case.a["arena"][:used], idx, fix=1, stats=stats)
        case._want["sim"] = (parsed, structs, stats)
    return case._want["sim"]


def parse_need(case):
    return len(parse_sim(case)[1])


def make_parse(n):
    from tests import _orc
    from tests.hevc_synth import annexb
    rng = np.random.default_rng(400 + n)
    m = {}
    for name, nals in nal_lists(n).items():
        assert len(nals) == n, (name, len(nals))
        idx, arena, _ = _orc.oracle().index_extract(np.frombuffer(annexb(nals), dtype=np.uint8))
        assert len(idx) == n, (name, len(idx))
        m[name] = S.Case("parse", "%d %s" % (n, name), dict(arena=arena, idx=idx, nals=nals))
    pad_input(rng, list(m.values()), "arena")
    return Family("parse %d" % n, "parse", m)


# ---- hbs_au_keep ---------------------------------------------------------------------------------------------------------------

KEEP_NALS, KEEP_AUS = 5 * 256 + 77, 200               # six workgroups of 256 NALs, the last one ragged


def make_keep():
    """the NALs of AUs [first, first + count) and the parameter sets in force in front of them: one count of NALs and of AUs, the AU
    boundaries and the parameter sets (with rc >= 0 and with rc < 0) elsewhere in each sibling; one sibling without any set in front"""
    rng = np.random.default_rng(420)
    m = {}
    for name in ("one", "two", "three", "no sets"):
        parsed = np.zeros(KEEP_NALS, dtype=AU.PARSED)
        parsed["nal_unit_type"] = rng.choice([0, 1, 19, 21, 32, 33, 34, 35, 39, 40], size=KEEP_NALS, p=[.2, .3, .05, .05, .06, .1, .1, .05, .05, .04])
        parsed["rc"] = np.where(rng.random(KEEP_NALS) < 0.3, -1, rng.integers(2, 900, KEEP_NALS))
        parsed["nal_temporal_id_plus1"] = 1
        parsed["struct_off"] = AU.NO_SLOT
        nal_au = au_cuts(rng, KEEP_NALS, KEEP_AUS)
        if name == "no sets":
            front = nal_au < 60
            parsed["nal_unit_type"][front & (parsed["nal_unit_type"] >= 32) & (parsed["nal_unit_type"] <= 34)] = 39
        m[name] = S.Case("keep", name, dict(nal_au=nal_au, parsed=parsed, first=60, count=90, param_sets=1))
    return Family("keep", "keep", m)


# ---- hbs_parse_extended --------------------------------------------------------------------------------------------------------

EXT_NALS = 2 * 256 + 91                                # three workgroups of 256 NALs, the last one ragged
NOT_EXTENDED = -99                                     # in place of an rc: hbs_parse_extended leaves that NAL's record alone


def ext_reference(nals):
    """-> (rc per NAL or NOT_EXTENDED, the hbs_ext_nal records: zeros for the NALs that are not of the types 35..40)"""
    from tests import _orc
    from tests.test_ext_types import EXT, oracle_ext
    rcs, recs = np.full(len(nals), NOT_EXTENDED, dtype=np.int64), np.zeros(len(nals), dtype=EXT)
    for k, nal in enumerate(nals):
        rc, t, rec = oracle_ext(_orc.oracle(), nal)
        if rc != -2 and t >= 0:
            rcs[k], recs[k] = rc, rec
    return rcs, recs


def make_ext():
    """the NAL mix of tests/test_ext_types.py::test_gpu_parse_extended_against_the_oracle cut to one count: the reference's golden
    vectors and random AUDs, EOS, EOB, filler data and SEI NALs with parameter sets and slices in between, drawn anew for each"""
    import json
    import os
    import random
    from tests import _orc
    from tests.hevc_synth import annexb
    from tests.test_ext_types import HERE, random_nals
    from tests.test_sim_parse_logic import sequence
    vec = [bytes.fromhex(v["nal"]) for v in json.load(open(os.path.join(HERE, "golden", "ext_vectors.json")))["vectors"]]
    pad = np.random.default_rng(440)
    m = {}
    for j, name in enumerate(("one", "two", "three", "four")):
        rng = random.Random(50 + j)
        pool = vec + random_nals(13 + j, 1200)
        rng.shuffle(pool)
        nals = []
        for nal in pool:                               # (a NAL must survive as one NAL inside an Annex-B stream: see that test)
            if len(nal) < 2 or nal[-1] == 0 or b"\x00\x00\x00" in nal or b"\x00\x00\x01" in nal or b"\x00\x00\x02" in nal:
                continue
            nals.append(nal)
            if rng.random() < 0.1:
                nals += sequence(rng.randrange(50))[:4]
        nals = nals[:EXT_NALS]
        idx, arena, _ = _orc.oracle().index_extract(np.frombuffer(annexb(nals), dtype=np.uint8))
        assert len(nals) == EXT_NALS == len(idx), (name, len(nals), len(idx))
        m[name] = S.Case("ext", name, dict(arena=arena, idx=idx, nals=nals))
    pad_input(pad, list(m.values()), "arena")
    return Family("ext", "ext", m)


PARSE_LARGE, PARSE_FEW = 300, 60

MAKERS = {"tsd": make_tsd, "tsm": make_tsm, "ins": make_ins, "keep": make_keep, "ext": make_ext, "emit pinned": make_emit_pinned, "emit auto": make_emit_auto, "emit tiny": make_emit_tiny,
          "parse large": lambda: make_parse(PARSE_LARGE), "parse few": lambda: make_parse(PARSE_FEW)}
for _w in ("small", "large"):
    MAKERS["a2l " + _w] = lambda w=_w: make_a2l(w)
    MAKERS["l2a " + _w] = lambda w=_w: make_l2a(w)
    MAKERS["flt " + _w] = lambda w=_w: make_flt(w)
# every family, as (name, packet size)
FAMILIES = [(k, 188) for k in MAKERS if k not in ("tsd", "tsm")] + [(k, B) for k in ("tsd", "tsm") for B in PACKET_SIZES]


def family_id(p):
    return "%s-%d" % p if p[0] in ("tsd", "tsm") else p[0].replace(" ", "-")
