"""The inputs of tests/test_gpu_sequences.py: for each of the five framing and transport calls a small, a large and an odd case
and an empty one, each good case with three variants (one malformed entry in the first plan workgroup, one in the last, an
output one byte short), and what the plain loops of tests/_*_ref.py say about every one of them.  numpy only: tests/test_seq_cases.py
holds the block counts and the expected errors on the CPU, so that the GPU tests cannot run on degenerate inputs.

A case is a Case: `a` holds the call's arguments (host arrays and numbers), `caps` the capacities a run is given, `room` what
the outputs of a run hold in front of their canaries (the needs of the good case the variant was made from), `bad` the edited
entry of a malformed variant.  want(case) is the reference's answer to a run, want(case, plan=True) to a plan."""
import numpy as np

from tests import _auins_ref as INS
from tests import _filter_ref as F
from tests import _lenpref_ref as LP
from tests import _ts_ref as TSD
from tests import _tsmux_ref as TSM
from tests.test_gpu_lenpref import random_aus
from tests.test_gpu_ts import FAULTS

CALLS = ("a2l", "l2a", "tsd", "tsm", "ins")          # annexb_to_lenpref, lenpref_to_annexb, ts_demux, ts_mux, au_insert
SIZES = ("small", "large", "odd")
VARIANTS = ("bad_early", "bad_late", "short")
E_ARG, E_CAPACITY = -3, -4
# items of a plan workgroup (hbs_lenpref.h, hbs_ts.h, hbs_tsmux.h: kTsmAusPerBlock = kTsmPlanLanes * kTsmPlanPer, hbs_auins.h)
NAL_BLOCK, SAMPLE_BLOCK, PACKET_BLOCK, TSM_AU_BLOCK, INS_AU_BLOCK = 2048, 256, 2048, 256, 256
TSM_COPY_BLOCK = 2048                                 # output packets of a copy workgroup of hbs_ts_mux
PID = 0x100


class Case:
    def __init__(self, call, name, a, bad=None):
        self.call, self.name, self.a, self.bad = call, name, a, bad
        self.caps, self.room = {}, {}
        self._want = {}

    def __repr__(self):
        return "%s %s" % (self.call, self.name)


def blocks(n, per):
    return (n + per - 1) // per


def items(case):
    """what the call's plan kernels count -> a tuple of (items, items per plan workgroup)"""
    a = case.a
    if case.call == "a2l":
        return ((len(a["idx"]), NAL_BLOCK),)
    if case.call == "l2a":
        return ((len(a["off"]), SAMPLE_BLOCK),)
    if case.call == "tsd":
        return ((len(a["ts"]) // a["B"], PACKET_BLOCK),)
    if case.call == "tsm":
        return ((len(a["au"]), TSM_AU_BLOCK),)
    return ((len(a["index"]), NAL_BLOCK), (len(a["au"]), INS_AU_BLOCK))


def plan_blocks(case):
    return tuple(blocks(n, per) for n, per in items(case))


def reference(case, plan=False):
    """the plain loop on the case's arguments (a plan looks at no capacity)"""
    a, c = case.a, ({} if plan else case.caps)
    if case.call == "a2l":
        return LP.to_lenpref_ref(a["s"], a["idx"], a["keep"], a["L"], a["nal_au"], a["n_aus"], c.get("out_cap"))
    if case.call == "l2a":
        return LP.to_annexb_ref(a["data"], a["off"], a["size"], a["L"], a["sc"], c.get("nal_cap"), c.get("out_cap"))
    if case.call == "tsd":
        return TSD.demux(a["ts"], a["B"], a["pid"], c.get("out_cap"), c.get("pes_cap"))
    if case.call == "tsm":
        return TSM.mux(a["stream"], a["au"], a["pts"], a["dts"], a["prm"], c.get("out_cap"))
    return INS.au_insert(a["stream"], a["index"], a["parsed"], a["au"], a["nal_au"], a["first"], a["count"], a["flags"],
                         c.get("out_cap"), c.get("index_cap"))


def want(case, plan=False):
    """reference(), computed once: the tests share it and leave it unchanged"""
    if plan not in case._want:
        case._want[plan] = reference(case, plan)
    return case._want[plan]


def summary_of(case, plan=False):
    return want(case, plan)[-1]


def reserved0(s):
    """reserved[0] of a reference summary (tests/_lenpref_ref.py keeps it as "reserved0", and only for the way back)"""
    return s["reserved"][0] if "reserved" in s else s.get("reserved0", 0)


def needs(case):
    """capacities of exactly what the good case puts out, from the reference's plan"""
    w = want(case, plan=True)
    s = w[-1]
    assert s["error"] == 0, (case, s)
    if case.call == "a2l":
        return dict(out_cap=s["stream_bytes"]), dict(out=s["stream_bytes"], io=s["nal_count"] * 32, so=(case.a["n_aus"] + 1) * 8)
    if case.call == "l2a":
        return dict(out_cap=s["stream_bytes"], nal_cap=s["nal_count"]), dict(out=s["stream_bytes"], so=(len(case.a["off"]) + 1) * 8)
    if case.call == "tsd":
        return dict(out_cap=s["stream_bytes"], pes_cap=s["nal_count"]), dict(out=s["stream_bytes"], pes=s["nal_count"] * 32)
    if case.call == "tsm":
        return dict(out_cap=s["stream_bytes"]), dict(out=s["stream_bytes"], ap=(len(case.a["au"]) + 1) * 4)
    M, cnt = s["nal_count"], s["reserved"][2]
    return dict(out_cap=s["stream_bytes"], index_cap=M), dict(out=s["stream_bytes"], io=M * 32, src=M * 4, nau=M * 4, auo=cnt * 64)


def finish(case):
    case.caps, case.room = needs(case)
    return case


# ---- the good cases -----------------------------------------------------------------------------------------------------------

def indexed_stream(rng, n, mean):
    """a random Annex-B stream and a consistent index of exactly n NALs.  The oracle's walk of a random stream ends at its first
    empty NAL, a few dozen NALs in: the stream is pieces of 4000 bytes, each cut behind the last NAL the oracle found in it,
    the entries moved by where the piece begins; some bytes no entry covers follow the last NAL."""
    from tests import _orc
    parts, entries, at, roff = [], [], 0, 0
    while sum(len(e) for e in entries) < n:
        s = F.random_stream(rng, 4000, mean)
        idx, _, _ = _orc.oracle().index_extract(s)
        if len(idx) == 0:
            continue
        cut = int(idx["end"][-1])
        idx["start"] += at
        idx["end"] += at
        idx["rbsp_off"] += roff
        parts.append(s[:cut])
        entries.append(idx)
        at, roff = at + cut, roff + int(idx["rbsp_len"].sum())
    idx = np.concatenate(entries)[:n]
    s = np.concatenate(parts)[: int(idx["end"][-1])]
    assert F.consistent(idx, len(s))
    return np.concatenate([s, rng.integers(1, 256, size=int(rng.integers(0, 9)), dtype=np.uint8)]), idx


def au_numbers(rng, n, lo, hi):
    """random_aus with lo..hi AUs, no multiple of the sample block but for a single one"""
    for _ in range(2000):
        au, n_aus = random_aus(rng, n)
        if lo <= n_aus <= hi and (n_aus % SAMPLE_BLOCK or n_aus == SAMPLE_BLOCK):
            return au, n_aus
    raise AssertionError("no AU numbering of %d..%d AUs" % (lo, hi))


# NALs and samples of the length-prefix cases: one plan workgroup of either call; four and more of the forward call with a ragged
# last one and three and more of the way back; between them, with 2-byte lengths and 3-byte start codes
A2L = dict(small=dict(mean=60, nals=700, aus=(2, SAMPLE_BLOCK), L=4, sc=4, keep=0.6),
           large=dict(mean=80, nals=3 * NAL_BLOCK + 517, aus=(3 * SAMPLE_BLOCK + 1, 1 << 20), L=4, sc=4, keep=0.6),
           odd=dict(mean=100, nals=NAL_BLOCK + 900, aus=(SAMPLE_BLOCK + 1, 2 * SAMPLE_BLOCK - 1), L=2, sc=3, keep=None))


def make_a2l(which, seed):
    p = A2L[which]
    rng = np.random.default_rng(seed)
    s, idx = indexed_stream(rng, p["nals"], p["mean"])
    nal_au, n_aus = au_numbers(rng, len(idx), *p["aus"])
    keep = (rng.random(len(idx)) < p["keep"]) if p["keep"] is not None else None
    if keep is not None:                           # only a kept NAL has to fit its length field
        keep &= (idx["end"] - idx["start"]) < (1 << (8 * p["L"]))
    else:
        assert int((idx["end"] - idx["start"]).max()) < (1 << (8 * p["L"]))
    return finish(Case("a2l", which, dict(s=s, idx=idx, keep=keep, L=p["L"], nal_au=nal_au, n_aus=n_aus)))


def make_l2a(which, seed):
    """the samples of the forward case's output, by its sample table"""
    fw = case("a2l", which, seed)
    out, _, so, _ = want(fw)
    so = so.astype(np.int64)
    return finish(Case("l2a", which, dict(data=out, off=so[:-1].astype(np.uint64), size=np.diff(so).astype(np.uint64), L=fw.a["L"], sc=A2L[which]["sc"])))


def make_tsd(which, seed, B):
    rng = np.random.default_rng(seed)
    if which == "odd":                             # another packet size, another PID, most packets of other PIDs, breaks
        B = TSD.SIZES[(TSD.SIZES.index(B) + 1) % 3]
        ts = TSD.random_ts(rng, PACKET_BLOCK + 300, B, 0x1E1, share=0.4, first_pes=PACKET_BLOCK + 5, p_break=0.05, p_pes=0.15)
        return finish(Case("tsd", which, dict(ts=ts.reshape(-1), B=B, pid=0x1E1)))
    # five blocks in the large case: the scratch is carved in units of 256 bytes and a block has 64 bytes of it, so up to four
    # blocks hold what one does, and tests/test_gpu_scratch.py wants the large case to hold more than the small one
    n = 1000 if which == "small" else 4 * PACKET_BLOCK + 7
    ts = TSD.random_ts(rng, n, B, PID, share=0.9, first_pes=2, p_break=0.02)
    return finish(Case("tsd", which, dict(ts=ts.reshape(-1), B=B, pid=PID)))


def make_tsm(which, seed, B):
    rng = np.random.default_rng(seed)
    if which == "odd":                             # another packet size, PSI in front of every IRAP AU, other counters and PIDs
        B = TSM.SIZES[(TSM.SIZES.index(B) + 1) % 3]
        prm = TSM.params(packet_bytes=B, flags=TSM.PCR | TSM.PSI_AT_IRAP, pid=0x1E1, pmt_pid=0x20, cc_es=11, cc_pat=14, cc_pmt=15, pcr_lead=9000)
        n, max_es = 2 * TSM_AU_BLOCK + 100, 300
    else:
        prm = TSM.params(packet_bytes=B, flags=TSM.PCR, cc_es=5)
        n, max_es = (200, 300) if which == "small" else (9 * TSM_AU_BLOCK + 37, 600)
    stream, au, pts, dts = TSM.random_case(rng, n, prm, max_es=max_es)
    return finish(Case("tsm", which, dict(stream=stream, au=au, pts=pts, dts=dts, prm=prm)))


def make_ins(which, seed):
    rng = np.random.default_rng(seed)
    n, flags, kw = dict(small=(200, 7, dict(irap_every=6)), large=(1700, 7, dict(irap_every=6)),
                        odd=(500, INS.AUD | INS.PARAM_SETS_FIRST, dict(irap_every=3, max_slices=5, p_aud=0.5)))[which]
    stream, index, parsed, compact, au, nal_au = INS.random_case(rng, n, **kw)
    return finish(Case("ins", which, dict(stream=stream, index=index, parsed=parsed, compact=compact, au=au, nal_au=nal_au,
                                          first=0, count=n, flags=flags)))


MAKERS = dict(a2l=make_a2l, l2a=make_l2a, tsd=make_tsd, tsm=make_tsm, ins=make_ins)
PACKET_CALLS = ("tsd", "tsm")                        # their cases take a packet size
_cases = {}


def case(call, which, seed=1, B=188):
    """the good case `which` of `call` (built once a process)"""
    key = (call, which, seed, B if call in PACKET_CALLS else None)
    if key not in _cases:
        _cases[key] = MAKERS[call](which, seed, B) if call in PACKET_CALLS else MAKERS[call](which, seed)
    return _cases[key]


def demux_of(mux):
    """hbs_ts_demux of what the hbs_ts_mux case puts out (by the reference), of the multiplexer's PID"""
    key = (id(mux), "demux")
    if key not in _cases:
        prm = mux.a["prm"]
        _cases[key] = finish(Case("tsd", "of the %s mux" % mux.name, dict(ts=want(mux)[0], B=prm["packet_bytes"], pid=prm["pid"])))
    return _cases[key]


def empty(call, B=188):
    """no NALs, samples, packets or AUs"""
    key = (call, "empty", B if call in PACKET_CALLS else None)
    if key in _cases:
        return _cases[key]
    z8 = np.zeros(0, dtype=np.uint8)
    if call == "a2l":
        a = dict(s=z8, idx=np.zeros(0, dtype=F.NAL_ENTRY), keep=None, L=4, nal_au=np.zeros(0, dtype=np.uint32), n_aus=0)
    elif call == "l2a":
        a = dict(data=z8, off=np.zeros(0, dtype=np.uint64), size=np.zeros(0, dtype=np.uint64), L=4, sc=4)
    elif call == "tsd":
        a = dict(ts=z8, B=B, pid=PID)
    elif call == "tsm":
        a = dict(stream=z8, au=np.zeros(0, dtype=TSM.ACCESS_UNIT), pts=np.zeros(0, dtype=np.uint64), dts=np.zeros(0, dtype=np.uint64),
                 prm=TSM.params(packet_bytes=B, flags=TSM.PCR))
    else:                                          # a stream and AUs, but no NALs (tests/test_gpu_auins.py::test_no_nals_or_no_aus)
        g = case("ins", "small").a
        a = dict(g, index=g["index"][:0], parsed=g["parsed"][:0], compact=g["compact"][:0], nal_au=g["nal_au"][:0])
    _cases[key] = finish(Case(call, "empty", a))
    return _cases[key]


# ---- the variants -------------------------------------------------------------------------------------------------------------

def edited_entry(good, late):
    """the entry a malformed variant edits: in the first plan workgroup, or in the last one (of the AU side for hbs_au_insert)"""
    n, per = items(good)[-1]
    if not late:
        return min(5, n - 1)
    return max(n - 3, (blocks(n, per) - 1) * per)


def malformed(good, late):
    """one entry edited as the calls' own tests edit theirs"""
    a = dict(good.a)
    at = edited_entry(good, late)
    if good.call == "a2l":                         # test_gpu_lenpref.py: an inconsistent index
        idx = a["idx"].copy()
        if late:
            idx["start"][at] = idx["end"][at - 1] - 1
        else:
            idx["start"][at] = idx["end"][at] + 1
        assert not F.consistent(idx, len(a["s"]))
        a["idx"] = idx
    elif good.call == "l2a":                       # test_gpu_lenpref.py: a sample a byte short of its last record
        size = a["size"].copy()
        full = np.flatnonzero(size > 8)
        at = int(full[-1]) if late else int(full[0])
        size[at] -= 1
        a["size"] = size
    elif good.call == "tsd":                       # test_gpu_ts.py: FAULTS
        B = a["B"]
        ts = a["ts"].copy().reshape(-1, B)
        t = ts[at, TSD.lead(B):]
        FAULTS["PTS without room" if late else "afl 184"](t)
        t[1], t[2] = (t[1] & 0xE0) | (a["pid"] >> 8), a["pid"] & 0xFF          # (the edits are written for PID 0x100)
        a["ts"] = ts.reshape(-1)
    elif good.call == "tsm":                       # test_gpu_tsmux.py::test_malformed_entries_and_times
        if late:
            pts = a["pts"].copy()
            pts[at] = 1 << 33
            a["pts"] = pts
        else:
            au = a["au"].copy()
            au["unit_begin"][at] = au["unit_end"][at] + 1
            a["au"] = au
    else:                                          # test_gpu_auins.py::test_inconsistent_tables
        if late:
            nal_au = a["nal_au"].copy()
            nal_au[int(a["au"]["first_nal"][at])] = at + 1
            a["nal_au"] = nal_au
        else:
            au = a["au"].copy()
            au["nal_count"][at] += 1
            a["au"] = au
    v = Case(good.call, good.name + (" bad-late" if late else " bad-early"), a, bad=at)
    v.caps, v.room = dict(good.caps), dict(good.room)
    return v


def short(good):
    """the good case with room for one byte less than it puts out"""
    v = Case(good.call, good.name + " short", good.a)
    v.caps, v.room = dict(good.caps, out_cap=good.caps["out_cap"] - 1), dict(good.room)
    return v


def variant(good, what):
    key = (id(good), what)
    if key not in _cases:
        _cases[key] = short(good) if what == "short" else malformed(good, what == "bad_late")
    return _cases[key]


def names_the_entry(call):
    """does the call's summary name the lowest entry in error?  The header gives reserved[0] = 1 + that entry to
    hbs_lenpref_to_annexb, hbs_ts_demux and hbs_ts_mux; hbs_annexb_to_lenpref leaves it 0, and hbs_au_insert's reserved[]
    counts what it inserted, so both are 0 under HBS_E_ARG."""
    return call in ("l2a", "tsd", "tsm")


def sequence(call, seed=1, B=188):
    """the ten steps of the sequence on one context -> [(case, plan only?)]"""
    small, large, odd = (case(call, w, seed, B) for w in SIZES)
    return [(large, False), (small, False), (variant(large, "bad_late"), False), (small, False), (variant(small, "bad_early"), False),
            (odd, False), (empty(call, B), False), (variant(large, "short"), False), (large, True), (large, False)]
