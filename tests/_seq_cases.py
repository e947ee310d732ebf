"""The inputs of tests/test_gpu_sequences.py: for each of the five framing and transport calls a small, a large and an odd case
and an empty one, each good case with three variants (one malformed entry in the first plan workgroup, one in the last, an
output one byte short), and what the plain loops of tests/_*_ref.py say about every one of them.  numpy only: tests/test_seq_cases.py
holds the block counts and the expected errors on the CPU, so that the GPU tests cannot run on degenerate inputs.

A case is a Case: `a` holds the call's arguments (host arrays and numbers), `caps` the capacities a run is given, `room` what
the outputs of a run hold in front of their canaries (the needs of the good case the variant was made from), `bad` the edited
entry of a malformed variant.  want(case) is the reference's answer to a run, want(case, plan=True) to a plan.

CALLS2 are the seven calls that came later, for tests/test_gpu_sequences_rtp_mp4.py: hbs_rtp_pack without and with
HBS_RTP_AGGREGATE, hbs_rtp_unpack, hbs_rtp_order, hbs_mp4_fragment, hbs_mp4_samples, hbs_mp4_stbl_samples and hbs_mp4_stbl_write.
Their scratch is laid out by capacities of the caller as well, so they have a variant a capacity that is one short (SHORTS) and
a "roomy" variant with every capacity well above the need, whose outputs are as large as the capacities (`spare`: the room behind
what is written).  A malformed variant of theirs says which summary word names the fault and with what (`named`), whether a plan
looks for it (`in_plan`) and which table the edited entry lies in (`among`).  order_of, unpack_of, samples_of and stbl_of are the
later stages of the pipelines, each on what the reference says the stage in front puts out.

CALLS3 are the timing and encryption calls, for tests/test_gpu_sequences_times_crypt.py: hbs_au_times, hbs_cenc_subsamples,
hbs_cenc_crypt and hbs_cbcs_crypt in both directions.  Only hbs_cenc_subsamples takes a capacity, so only it has a short and a
roomy variant; the crypt calls have no plan, one set of tables a size between them, and a fourth table in which no sample has an
entry (hollow).  Their section is at the end of the file."""
import numpy as np

from tests import _au_times_ref as T
from tests import _auins_ref as INS
from tests import _cbcs_ref as CB
from tests import _cenc_ref as CR
from tests import _filter_ref as F
from tests import _lenpref_ref as LP
from tests import _mp4_read_ref as MR
from tests import _mp4_ref as MF
from tests import _mp4_stbl_ref as MS
from tests import _mp4_stbl_write_ref as MW
from tests import _rtp_ap_ref as RA
from tests import _rtp_order_ref as RO
from tests import _rtp_ref as R
from tests import _rtp_unpack_ref as RU
from tests import _ts_ref as TSD
from tests import _tsmux_ref as TSM
from tests.test_gpu_lenpref import random_aus
from tests.test_gpu_mp4_read import moofs_of
from tests.test_gpu_mp4_stbl import case as stbl_case, track as stbl_track
from tests.test_gpu_ts import FAULTS

CALLS = ("a2l", "l2a", "tsd", "tsm", "ins")          # annexb_to_lenpref, lenpref_to_annexb, ts_demux, ts_mux, au_insert
SIZES = ("small", "large", "odd")
VARIANTS = ("bad_early", "bad_late", "short")
E_ARG, E_CAPACITY = -3, -4
# items of a plan workgroup (hbs_lenpref.h, hbs_ts.h, hbs_tsmux.h: kTsmAusPerBlock = kTsmPlanLanes * kTsmPlanPer, hbs_auins.h)
NAL_BLOCK, SAMPLE_BLOCK, PACKET_BLOCK, TSM_AU_BLOCK, INS_AU_BLOCK = 2048, 256, 2048, 256, 256
TSM_COPY_BLOCK = 2048                                 # output packets of a copy workgroup of hbs_ts_mux
PID = 0x100
# the RTP calls, after CALLS: hbs_rtp_pack without and with HBS_RTP_AGGREGATE, hbs_rtp_unpack, hbs_rtp_order
RTP_CALLS = ("rtp", "rtpa", "rtpu", "rtpo")
# ... and the MP4 calls: hbs_mp4_fragment, hbs_mp4_samples, hbs_mp4_stbl_samples, hbs_mp4_stbl_write
MP4_CALLS = ("mp4f", "mp4s", "stbl", "stblw")
CALLS2 = RTP_CALLS + MP4_CALLS
# items of a plan workgroup (hbs_rtp.h: kRtpNalsPerBlock = kRtpPlanLanes, hbs_rtpun.h: kRtpuPacketsPerBlock, hbs_rtpord.h:
# kRtpoLanes, a lane a packet or a lane a slot) and the output bytes of a copy workgroup (hbs_rtp.h: kRtpTileBytes; hbs_rtp_unpack
# copies through the piece table, whose tiles are as large)
RTP_NAL_BLOCK, RTPU_PACKET_BLOCK, RTPO_BLOCK = 256, 256, 256
TILE = 64 * 1024
# hbs_mp4.h: kMp4NalsPerBlock = kMp4Lanes * kMp4NalsPer, kMp4AusPerBlock = kMp4Lanes, kMp4TileBytes = 64 KiB; hbs_mp4rd.h: kRdLanes
# (segments, moofs and samples); hbs_mp4stbl.h: kStLanes (table entries and samples); hbs_mp4stblw.h: kSwLanes (samples, chunks, runs)
MP4_NAL_BLOCK, MP4_AU_BLOCK, MP4RD_BLOCK, STBL_BLOCK, STBLW_BLOCK = 256, 256, 256, 256, 256
ROOM_ITEMS, ROOM_BYTES = 3 * 256 + 1, TILE + 1        # what a roomy variant gives a counted and a byte capacity above the need
# the capacities a run is given one short, a variant each; "short_span" is hbs_rtp_order's max_span
SHORTS = dict(rtp=("short",), rtpa=("short",), rtpu=("short", "short_nal", "short_au"), rtpo=("short", "short_span"),
              mp4f=("short", "short_frag"), mp4s=("short_moof", "short_sample"), stbl=("short_sample",), stblw=("short",))
SHORT_CAP = dict(short="out_cap", short_nal="nal_cap", short_au="au_cap", short_frag="frag_cap", short_moof="moof_cap",
                 short_sample="sample_cap")
PLAN_SHORT = ("short_span", "short_moof")             # capacities a plan looks at as well: max_span, moof_cap
# the timing and encryption calls, for tests/test_gpu_sequences_times_crypt.py: hbs_au_times, hbs_cenc_subsamples, hbs_cenc_crypt,
# hbs_cbcs_crypt encrypting and with HBS_CBCS_DECRYPT
CRYPT_CALLS = ("cenc", "cbcs", "cbcsd")
CALLS3 = ("aut", "csub") + CRYPT_CALLS
# hbs_autimes.h: kAutLanes, kAutHalo; hbs_cenc.h: kCencNalsPerBlock, a lane a sample of kPlanLanes, kCencRanges; hbs_cbcs.h: kCbcsLaneBlocks
AUT_BLOCK, AUT_HALO, CENC_NAL_BLOCK, CRYPT_SAMPLE_BLOCK, CRYPT_RANGES, CBCS_LANE_BLOCKS = 256, 64, 2048, 256, 1024, 64
E_DEPTH = -6
AUT_TABLES = (("dts", 8), ("pts", 8), ("order", 4), ("display", 4))          # d_dts, d_pts, d_order, d_display and their entries' bytes
CRYPT_TAIL = 37                                       # bytes of the data buffer behind the last sample
SHORTS["csub"] = ("short",)
SHORT_CAP["csub"] = "sub_cap"                         # (hbs_cenc_subsamples' only capacity: by the call, not by the variant's name)


class Case:
    def __init__(self, call, name, a, bad=None):
        self.call, self.name, self.a, self.bad = call, name, a, bad
        self.caps, self.room = {}, {}
        self.spare = {}                                # output -> the bytes of room behind what a roomy variant writes
        # a malformed variant: the summary word that names the fault and its value (1 + bad, or 1 + the box for a table error of
        # hbs_mp4_stbl_samples); does a plan find the fault; (items, items per workgroup) of the table the edited entry lies in
        self.named, self.in_plan, self.among = None, True, None
        self.error = E_ARG                             # the error of a malformed variant (hbs_au_times: HBS_E_DEPTH)
        self._want = {}

    def __repr__(self):
        return "%s %s" % (self.call, self.name)


def blocks(n, per):
    return (n + per - 1) // per


def items(case):
    """what the call's plan kernels count -> a tuple of (items, items per plan workgroup)"""
    a = case.a
    if case.call == "aut":
        return ((len(a["au"]), AUT_BLOCK),)
    if case.call == "csub":
        return ((len(a["index"]), CENC_NAL_BLOCK),)
    if case.call in CRYPT_CALLS:                   # the samples, and the entries by the thousand: the kernels walk them in 1 024 ranges
        return ((len(a["off"]), CRYPT_SAMPLE_BLOCK), (crypt_entries(a), CRYPT_RANGES))
    if case.call in ("rtp", "rtpa"):
        return ((len(a["index"]), RTP_NAL_BLOCK),)
    if case.call == "rtpu":
        return ((len(a["off"]), RTPU_PACKET_BLOCK),)
    if case.call == "rtpo":                        # the packets, and the slots of the span the call finds
        return ((len(a["off"]), RTPO_BLOCK), (want(case, plan=True)[-1]["stream_bytes"], RTPO_BLOCK))
    if case.call == "mp4f":
        return ((len(a["index"]), MP4_NAL_BLOCK), (len(a["au"]), MP4_AU_BLOCK))
    if case.call == "mp4s":                        # moofs and samples (the segments: tests/test_seq_cases.py)
        s = want(case, plan=True)[-1]
        return ((s["nal_found"], MP4RD_BLOCK), (s["nal_count"], MP4RD_BLOCK))
    if case.call == "stbl":                        # samples, and the entries of the longest of stsc, stts, ctts, stss
        return ((want(case, plan=True)[-1]["nal_count"], STBL_BLOCK), (max(stbl_entries(a["rec"]).values()), STBL_BLOCK))
    if case.call == "stblw":                       # samples, chunks, the runs of the stts
        w = want(case, plan=True)
        return ((w[-1]["nal_count"], STBLW_BLOCK), (w[-1]["nal_found"], STBLW_BLOCK), (stbl_entries(w[1].view(MS.STBL))["stts"], STBLW_BLOCK))
    if case.call == "a2l":
        return ((len(a["idx"]), NAL_BLOCK),)
    if case.call == "l2a":
        return ((len(a["off"]), SAMPLE_BLOCK),)
    if case.call == "tsd":
        return ((len(a["ts"]) // a["B"], PACKET_BLOCK),)
    if case.call == "tsm":
        return ((len(a["au"]), TSM_AU_BLOCK),)
    return ((len(a["index"]), NAL_BLOCK), (len(a["au"]), INS_AU_BLOCK))


def stbl_entries(rec):
    """the entries of stsc, stts, ctts and stss by the bytes of their payloads"""
    return {name: max(int(rec[name][0][1]) - 8, 0) // per for name, per in (("stsc", 12), ("stts", 8), ("ctts", 8), ("stss", 4))}


def plan_blocks(case):
    return tuple(blocks(n, per) for n, per in items(case))


def reference(case, plan=False):
    """the plain loop on the case's arguments (a plan looks at no capacity)"""
    a, c = case.a, ({} if plan else case.caps)
    if case.call in CALLS3:
        return reference3(case, plan)
    if case.call in ("rtp", "rtpa"):
        return RA.pack(a["stream"], a["index"], a["nal_au"], a["n_aus"], a["pts"], a["prm"], c.get("out_cap"))
    if case.call == "rtpu":
        r = RU.unpack(a["data"], a["off"], a["size"], a["prm"], c.get("out_cap"), c.get("nal_cap"), c.get("au_cap"))
        return r["out"], r["index"], r["nal_au"], r["au_ts"], r["summary"]
    if case.call == "rtpo":
        r = RO.order(a["data"], a["off"], a["size"], a["prm"], c.get("out_cap"))
        return r["off"], r["size"], r["src"], r["ext"], r["summary"]
    if case.call == "mp4f":
        return MF.fragment(a["stream"], a["index"], a["keep"], a["nal_au"], a["au"], a["dts"], a["pts"], a["prm"], c.get("out_cap"), c.get("frag_cap"))
    if case.call == "mp4s":                        # (moof_cap sizes the plan's scratch too, and the plan looks at it)
        return MR.samples(a["data"], a["segs"], a["prm"], moof_cap=case.caps.get("moof_cap"), sample_cap=c.get("sample_cap"), tables=not plan)
    if case.call == "stbl":
        return MS.read(a["data"], a["rec"], outputs=False) if plan else MS.read(a["data"], a["rec"], sample_cap=c.get("sample_cap"))
    if case.call == "stblw":                       # (a plan writes d_tables, and the reference gives the boxes all the same)
        blob, rec, s = MW.call(a, **({} if plan else dict(out_cap=c["out_cap"])))
        return (None if blob is None else np.frombuffer(blob, dtype=np.uint8)), (None if rec is None else rec.view(np.uint8).reshape(-1)), s
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
    if case.call in CALLS3:
        return needs3(case)
    w = want(case, plan=True)
    s = w[-1]
    assert s["error"] == 0, (case, s)
    if case.call in ("rtp", "rtpa"):
        n = len(case.a["index"])
        return dict(out_cap=s["stream_bytes"]), dict(out=s["stream_bytes"], no=(n + 1) * 8, npk=(n + 1) * 8)
    if case.call == "rtpu":
        nals, aus = s["nal_count"], s["reserved"][1]
        return dict(out_cap=s["stream_bytes"], nal_cap=nals, au_cap=aus), dict(out=s["stream_bytes"], io=nals * 32, nau=nals * 4, ats=aus * 8)
    if case.call == "rtpo":
        kept = s["nal_count"]
        return dict(out_cap=kept), dict(ooff=kept * 8, osize=kept * 8, src=kept * 4, ext=kept * 8)
    if case.call == "mp4f":
        m, frags = len(case.a["au"]), s["nal_count"]
        return dict(out_cap=s["stream_bytes"], frag_cap=frags), dict(out=s["stream_bytes"], so=m * 8, ss=m * 8, fr=frags * MF.FRAG.itemsize)
    if case.call == "mp4s":
        n, m = s["nal_count"], s["nal_found"]
        return dict(moof_cap=m, sample_cap=n), dict(so=n * 8, ss=n * 8, dts=n * 8, pts=n * 8, sfl=n * 4, fr=m * MF.FRAG.itemsize)
    if case.call == "stbl":
        n = s["nal_count"]
        return dict(sample_cap=n), dict(so=n * 8, ss=n * 8, dts=n * 8, pts=n * 8, sfl=n * 4)
    if case.call == "stblw":
        return dict(out_cap=s["stream_bytes"]), dict(out=s["stream_bytes"], tab=MS.STBL.itemsize)
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
    if case.call == "mp4s":                        # the plan's moof_cap is the count of a plan without a limit
        case.caps = dict(moof_cap=MR.samples(case.a["data"], case.a["segs"], case.a["prm"], tables=False)[-1]["nal_found"])
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


# NALs of the hbs_rtp_pack cases: one plan workgroup; three and a ragged fourth, the output across three copy tiles and more;
# between them with the other framing, another max_payload, HBS_RTP_OPEN_END and times by ts_step
RTP = dict(small=dict(n=200, max_nal=900, times=True, prm=R.params(max_payload=300, seq=65400, ts_base=0xFFFFFF00)),
           large=dict(n=3 * RTP_NAL_BLOCK + 57, max_nal=900, times=True, prm=R.params(max_payload=300, seq=65400, ts_base=0xFFFFFF00)),
           odd=dict(n=RTP_NAL_BLOCK + 100, max_nal=400, times=False, prm=R.params(max_payload=100, framing=2, flags=R.OPEN_END, seq=7, ts_step=3003)))
RTPA = dict(small=dict(n=200, max_nal=500, times=True, prm=R.params(max_payload=1188, flags=RA.AGGREGATE, seq=65400, ts_base=0xFFFFFF00)),
            large=dict(n=3 * RTP_NAL_BLOCK + 57, max_nal=500, times=True, prm=R.params(max_payload=1188, flags=RA.AGGREGATE, seq=65400, ts_base=0xFFFFFF00)),
            odd=dict(n=RTP_NAL_BLOCK + 100, max_nal=120, times=False,
                     prm=R.params(max_payload=100, framing=2, flags=RA.AGGREGATE | R.OPEN_END, seq=7, ts_step=3003)))


def make_rtp(which, seed, table=RTP, call="rtp"):
    p = table[which]
    rng = np.random.default_rng(seed + (300 if call == "rtp" else 400))
    stream, index, nal_au, n_aus, pts = R.random_case(rng, p["n"], max_nal=p["max_nal"], times=p["times"])
    return finish(Case(call, which, dict(stream=stream, index=index, nal_au=nal_au, n_aus=n_aus, pts=pts, prm=p["prm"])))


def make_rtpa(which, seed):
    return make_rtp(which, seed, RTPA, "rtpa")


# packets of the hbs_rtp_unpack cases (single NALs and whole FU chains; the odd case also aggregation packets, CSRC entries,
# header extensions, padding, 3-byte start codes and HBS_RTPU_MATCH_SSRC)
RTPU = dict(small=dict(n=200, hi=60, aps=False, odd_headers=False, prm=RU.params()),
            large=dict(n=3 * RTPU_PACKET_BLOCK + 57, hi=600, aps=False, odd_headers=False, prm=RU.params()),
            odd=dict(n=RTPU_PACKET_BLOCK + 100, hi=200, aps=True, odd_headers=True, prm=RU.params(startcode_bytes=3, flags=RU.MATCH_SSRC)))


def make_rtpu(which, seed):
    p = RTPU[which]
    rng = np.random.default_rng(seed + 500)
    packets, _, _, _ = RU.random_packets(rng, p["n"], lo=4, hi=p["hi"], odd_headers=p["odd_headers"], aps=p["aps"])
    data, off, size = RU.lay_out(packets, rng)
    return finish(Case("rtpu", which, dict(data=data, off=off, size=size, prm=p["prm"])))


# packets sent of the hbs_rtp_order cases, a tenth of them lost, shuffled inside a window, five arriving twice, one in twenty
# entries another stream's; the large case wraps its sequence numbers and has two packets displaced across workgroups; the odd
# case continues behind after_ext (its first eleven packets are late) and tells the other stream by its SSRC
RTPO = dict(small=dict(n=200, seq0=100, flags=0), large=dict(n=4 * RTPO_BLOCK + 91, seq0=65000, flags=0),
            odd=dict(n=400, seq0=65500, flags=RO.MATCH_SSRC | RO.AFTER))
RTPO_LATE = 11


def make_rtpo(which, seed):
    p = RTPO[which]
    rng = np.random.default_rng(seed + 600)
    n, seq0, W = p["n"], p["seq0"], RTPO_BLOCK
    packets = [RU.packet(RU.random_nal(rng, int(rng.integers(2, 29))), (seq0 + k) & 0xFFFF, 90 * k) for k in range(n)]
    lose = sorted(int(x) for x in rng.choice(np.arange(RTPO_LATE + 1, n - 1), size=n // 10, replace=False))
    arrived, _ = RO.arrive(packets, rng, window=8, duplicates=5, lose=lose, others=0.05, other_kind="ssrc" if p["flags"] & RO.MATCH_SSRC else "pt")
    if which == "large":                           # tests/test_gpu_rtp_order.py::test_displacement_across_workgroups
        arrived.insert(2 * W + 5, arrived.pop(5))
        arrived.insert(7, arrived.pop(3 * W + 9))
    data, off, size = RU.lay_out(arrived, rng)
    if p["flags"] & RO.AFTER:
        after = RO.START + 2 * 65536 + seq0 + RTPO_LATE - 1
        prm = RO.params(flags=p["flags"], after_ext=after, max_span=n - RTPO_LATE)
    else:                                          # one workgroup of slots; the span and part of a ragged workgroup more
        prm = RO.params(max_span=W if which == "small" else n + 37)
    return finish(Case("rtpo", which, dict(data=data, off=off, size=size, prm=prm)))


# AUs of the hbs_mp4_fragment cases (one to three or four NALs each): one workgroup of NALs and of AUs; four of AUs and more of
# NALs, both ragged, the output across three copy tiles and more; between them with 2-byte lengths, fragments of at most seven
# samples instead of a cut at every IRAP, and the caller's times
MP4F = dict(small=dict(aus=80, per_au=3, times=False, prm=MF.params(length_size=4, flags=MF.CUT_AT_IRAP, track_id=3, sequence=40, base_time=1 << 33)),
            large=dict(aus=3 * MP4_AU_BLOCK + 57, per_au=4, times=False,
                       prm=MF.params(length_size=4, flags=MF.CUT_AT_IRAP, track_id=3, sequence=40, base_time=1 << 33)),
            odd=dict(aus=MP4_AU_BLOCK + 100, per_au=2, times=True, prm=MF.params(length_size=2, max_samples=7, track_id=5, sequence=(1 << 32) - 2)))


def make_mp4f(which, seed):
    p = MP4F[which]
    rng = np.random.default_rng(seed + 700)
    stream, index, keep, nal_au, au, dts, pts = MF.random_case(rng, p["aus"], max_nal=300, max_nals_per_au=p["per_au"], times=p["times"], irap_every=30)
    return finish(Case("mp4f", which, dict(stream=stream, index=index, keep=keep, nal_au=nal_au, au=au, dts=dts, pts=pts, prm=p["prm"])))


# moofs of the hbs_mp4_samples cases, one to three samples in one trun each (the last moof: three samples, their sizes in the
# entries, a data_offset); the odd case is a table of segments of two moofs each, records of 24 bytes, other trex defaults
MP4S = dict(small=dict(moofs=100, per_seg=None, stride=16, prm=MR.read_params(track_id=1, trex_duration=7, trex_size=3, trex_flags=0x01010000)),
            large=dict(moofs=3 * MP4RD_BLOCK + 57, per_seg=None, stride=16,
                       prm=MR.read_params(track_id=1, trex_duration=7, trex_size=3, trex_flags=0x01010000)),
            odd=dict(moofs=MP4RD_BLOCK + 100, per_seg=2, stride=24, prm=MR.read_params(track_id=2, trex_duration=1000, trex_size=9)))


def make_mp4s(which, seed):
    p = MP4S[which]
    rng = np.random.default_rng(seed + 800)
    shapes = [[int(c)] for c in rng.integers(1, 4, size=p["moofs"] - 1)] + [[3]]
    tflags = [None] * (p["moofs"] - 1) + [[0x201]]
    buf, _, frags = moofs_of(rng, p["prm"], shapes, tflags, per_seg=p["per_seg"])
    segs = None
    if p["per_seg"]:                               # tests/test_gpu_mp4_read.py::test_moof_counts_around_a_workgroup
        cut = [int(f["out_off"]) for f in frags[::p["per_seg"]]] + [len(buf)]
        segs = [(a, b - a) for a, b in zip(cut, cut[1:])]
    moof_off = [int(f["out_off"]) for f in frags]
    return finish(Case("mp4s", which, dict(data=np.frombuffer(buf, dtype=np.uint8), segs=segs, stride=p["stride"], prm=p["prm"], moof_off=moof_off)))


# samples of the hbs_mp4_stbl_samples cases; the odd case has a co64, one sample size in the stsz and no stss
STBL = dict(small=dict(n=200, co64=False, constant=None, sync=True), large=dict(n=5000, co64=False, constant=None, sync=True),
            odd=dict(n=2200, co64=True, constant=33, sync=False))


def make_stbl(which, seed):
    p = STBL[which]
    t = stbl_track(np.random.default_rng(seed + 900), p["n"], constant=p["constant"])
    if not p["sync"]:
        t["sync"] = None
    buf, rec = stbl_case(t, co64=p["co64"], constant=p["constant"], first=(1 << 33) + 5 if p["co64"] else 0, lead=5)
    return finish(Case("stbl", which, dict(data=np.frombuffer(buf, dtype=np.uint8), rec=rec, t=t, co64=p["co64"], constant=p["constant"])))


# samples of the hbs_mp4_stbl_write cases; the odd case writes a co64 for offsets above 4 GiB and cuts its chunks every three samples
STBLW = dict(small=dict(n=200, params=dict()), large=dict(n=2600, params=dict()),
             odd=dict(n=900, params=dict(co64=True, max_chunk_samples=3, data_offset=(1 << 33) + 4)))


def make_stblw(which, seed):
    p = STBLW[which]
    t, _, dur = MW.random_tables(np.random.default_rng(seed + 1000), p["n"])
    return finish(Case("stblw", which, MW.case("%s %d" % (which, seed), t, sample_duration=dur, **p["params"])))


MAKERS = dict(a2l=make_a2l, l2a=make_l2a, tsd=make_tsd, tsm=make_tsm, ins=make_ins, rtp=make_rtp, rtpa=make_rtpa, rtpu=make_rtpu,
              rtpo=make_rtpo, mp4f=make_mp4f, mp4s=make_mp4s, stbl=make_stbl, stblw=make_stblw)
# (the makers of CALLS3 are added below, where they are defined)
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


def order_of(pack):
    """hbs_rtp_order of the packets the hbs_rtp_pack case puts out (by the reference), their table shuffled inside a window of
    eight on the host; max_span is the packets' number"""
    key = (id(pack), "order")
    if key not in _cases:
        out, nal_off, nal_packet, _ = want(pack)
        prm = pack.a["prm"]
        at = RA.packet_offsets(nal_off, nal_packet, prm)
        off, size = at[:-1] + np.uint64(prm["framing"]), np.diff(at) - np.uint64(prm["framing"])
        seen = RO.arrival_order(len(off), 8, np.random.default_rng(len(off)))
        _cases[key] = finish(Case("rtpo", "of the %s %s" % (pack.name, pack.call), dict(data=out, off=off[seen], size=size[seen],
                                                                                         prm=RO.params(flags=RO.MATCH_SSRC, max_span=len(off)))))
    return _cases[key]


def unpack_of(order):
    """hbs_rtp_unpack of the table the hbs_rtp_order case puts out (by the reference)"""
    key = (id(order), "unpack")
    if key not in _cases:
        off, size, _, _, _ = want(order)
        _cases[key] = finish(Case("rtpu", order.name, dict(data=order.a["data"], off=off, size=size, prm=RU.params(flags=RU.MATCH_SSRC))))
    return _cases[key]


def samples_of(frag):
    """hbs_mp4_samples of what the hbs_mp4_fragment case puts out (by the reference), as one segment"""
    key = (id(frag), "samples")
    if key not in _cases:
        out, _, _, frags, _ = want(frag)
        a = dict(data=out, segs=None, stride=16, prm=MR.read_params(track_id=frag.a["prm"]["track_id"]), moof_off=[int(x) for x in frags["out_off"]])
        _cases[key] = finish(Case("mp4s", "of the %s fragments" % frag.name, a))
    return _cases[key]


STBL_FILE_BYTES = 1 << 40                          # of the file the boxes of an hbs_mp4_stbl_write case describe: above every sample


def stbl_of(write):
    """hbs_mp4_stbl_samples of the boxes the hbs_mp4_stbl_write case puts out (by the reference), by the record it gives"""
    key = (id(write), "stbl")
    if key not in _cases:
        blob, rec, _ = want(write)
        rec = rec.view(MS.STBL).copy()
        rec["file_bytes"] = STBL_FILE_BYTES
        _cases[key] = finish(Case("stbl", "of the %s boxes" % write.name, dict(data=blob, rec=rec)))
    return _cases[key]


def empty(call, B=188):
    """no NALs, samples, packets or AUs"""
    key = (call, "empty", B if call in PACKET_CALLS else None)
    if key in _cases:
        return _cases[key]
    z8, z64 = np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint64)
    if call in CALLS3:
        a = empty3(call)
    elif call in ("rtp", "rtpa"):
        a = dict(stream=z8, index=np.zeros(0, dtype=R.NAL_ENTRY), nal_au=np.zeros(0, dtype=np.uint32), n_aus=0, pts=z64,
                 prm=(RTP if call == "rtp" else RTPA)["small"]["prm"])
    elif call == "rtpu":
        a = dict(data=z8, off=z64, size=z64, prm=RU.params())
    elif call == "rtpo":
        a = dict(data=z8, off=z64, size=z64, prm=RO.params(max_span=RTPO_BLOCK))
    elif call == "mp4f":
        a = dict(stream=z8, index=np.zeros(0, dtype=MF.NAL_ENTRY), keep=None, nal_au=np.zeros(0, dtype=np.uint32), au=np.zeros(0, dtype=MF.ACCESS_UNIT),
                 dts=None, pts=None, prm=MP4F["small"]["prm"])
    elif call == "mp4s":                           # an empty buffer as one segment
        a = dict(data=z8, segs=None, stride=16, prm=MP4S["small"]["prm"], moof_off=[])
    elif call == "stbl":                           # tests/test_gpu_mp4_stbl.py::test_sample_counts_around_a_workgroup: boxes of no entry
        t = stbl_track(np.random.default_rng(0), 0)
        buf, rec = stbl_case(t, lead=5)
        a = dict(data=np.frombuffer(buf, dtype=np.uint8), rec=rec, t=t, co64=False, constant=None)
    elif call == "stblw":
        a = MW.case("empty", MW.random_tables(np.random.default_rng(0), 0)[0])
    elif call == "a2l":
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
    n, per = edited_table(good, late)
    if not late:
        return min(5, n - 1)
    return max(n - 3, (blocks(n, per) - 1) * per)


def edited_table(good, late):
    """(items, items per workgroup) of the table a malformed variant edits: the NALs of hbs_rtp_pack and hbs_mp4_fragment, the
    packets of hbs_rtp_unpack and hbs_rtp_order, a moof (early) or a sample (late) of hbs_mp4_samples, a sample (early) or an
    stsc entry (late) of hbs_mp4_stbl_samples, a sample of hbs_mp4_stbl_write; of the five older calls the last side"""
    if good.call == "mp4s":
        return items(good)[1 if late else 0]
    if good.call == "stbl" and late:
        return stbl_entries(good.a["rec"])["stsc"], STBL_BLOCK
    return items(good)[0 if good.call in CALLS2 else -1]


def malformed(good, late):
    """one entry edited as the calls' own tests edit theirs"""
    if good.call in CALLS3:
        return malformed3(good, late)
    a = dict(good.a)
    at = edited_entry(good, late)
    word, value, in_plan = 0, None, True
    if good.call == "mp4f":                        # test_gpu_mp4.py::test_nal_errors: "start_gt_end", "overlap"
        index = a["index"].copy()
        index["start"][at] = index["end"][at - 1] - 1 if late else index["end"][at] + 1
        a["index"] = index
    elif good.call == "mp4s":                      # test_gpu_mp4_read.py::test_errors_at_the_stated_segment_moof_and_sample
        data = a["data"].copy()
        raw = data.tobytes()
        if late:                                   # a negative data begin in the last moof: a sample error at its first sample
            at, word = summary_of(good)["nal_count"] - 3, 2
            i = raw.index(b"trun", a["moof_off"][-1])
            data[i + 12:i + 16] = np.frombuffer((-(1 << 31)).to_bytes(4, "big", signed=True), dtype=np.uint8)
        else:                                      # no tfdt in moof `at`: a moof error
            word = 1
            i = raw.index(b"tfdt", a["moof_off"][at])
            assert i < a["moof_off"][at + 1]
            data[i:i + 4] = np.frombuffer(b"free", dtype=np.uint8)
        a["data"] = data
    elif good.call == "stbl":                      # test_gpu_mp4_stbl.py: a sample behind file_bytes; "a broken entry far down a table"
        rec = a["rec"].copy()
        if late:                                   # entry `at` of the stsc repeats the first_chunk of the entry in front: box 3
            assert at >= 1
            data = a["data"].copy()
            o = int(rec["stsc"][0][0]) + 8 + 12 * at
            data[o:o + 4] = data[o - 12:o - 8]
            a["data"], value = data, 3
        else:                                      # (a plan does not look for sample errors)
            off, size = want(good)[0], want(good)[1]
            at = int(np.flatnonzero(size[at:] > 0)[0]) + at
            rec["file_bytes"] = int(off[at]) + int(size[at]) - 1
            word, in_plan = 2, False
        a["rec"] = rec
    elif good.call == "stblw":                     # _mp4_stbl_write_ref.py::error_cases: "a size above 2^32 - 1", "a pts of 2^62"
        t = {k: (None if v is None else list(v)) for k, v in a["t"].items()}
        if late:
            t["pts"][at] = 1 << 62
        else:
            t["size"][at] = 1 << 32
        a["t"], word = t, 2
    elif good.call in ("rtp", "rtpa"):               # test_gpu_rtp.py::test_malformed_nals: "one byte", "type 48"
        if late:
            stream = a["stream"].copy()
            stream[int(a["index"]["start"][at])] = 48 << 1
            a["stream"] = stream
        else:
            index = a["index"].copy()
            index["end"][at] = index["start"][at] + 1
            a["index"] = index
    elif good.call in ("rtpu", "rtpo"):            # test_gpu_rtp_unpack.py, test_gpu_rtp_order.py: "version 1", a packet that leaves the buffer
        if late:
            data = a["data"].copy()
            data[int(a["off"][at])] = 0x40
            a["data"] = data
        else:
            size = a["size"].copy()
            size[at] = len(a["data"]) - int(a["off"][at]) + 1
            a["size"] = size
    elif good.call == "a2l":                       # test_gpu_lenpref.py: an inconsistent index
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
    if good.call in CALLS2:
        v.named, v.in_plan, v.among = (word, at + 1 if value is None else value), in_plan, edited_table(good, late)
    return v


def short(good, what="short"):
    """the good case with room for one byte, or one entry, less than it puts out: in out_cap, or in the capacity `what` names"""
    v = Case(good.call, good.name + " " + what.replace("_", " "), good.a)
    v.caps, v.room = dict(good.caps), dict(good.room)
    if what == "short_span":
        v.a = dict(good.a, prm=dict(good.a["prm"], max_span=summary_of(good)["stream_bytes"] - 1))
    else:
        v.caps[SHORT_CAP[good.call if good.call in CALLS3 else what]] -= 1
    return v


def roomy(good):
    """the good case with every capacity the caller gives well above the need: ROOM_BYTES more in a byte capacity, ROOM_ITEMS more
    in a counted one, a max_span of more than twice the large case's; the outputs are as large as the capacities"""
    v = Case(good.call, good.name + " roomy", good.a)
    per = dict(rtp=dict(out_cap=("out", 1)), rtpa=dict(out_cap=("out", 1)),
               rtpu=dict(out_cap=("out", 1), nal_cap=("io", 32, "nau", 4), au_cap=("ats", 8)),
               rtpo=dict(out_cap=("ooff", 8, "osize", 8, "src", 4, "ext", 8)),
               mp4f=dict(out_cap=("out", 1), frag_cap=("fr", MF.FRAG.itemsize)),
               mp4s=dict(moof_cap=("fr", MF.FRAG.itemsize), sample_cap=("so", 8, "ss", 8, "dts", 8, "pts", 8, "sfl", 4)),
               stbl=dict(sample_cap=("so", 8, "ss", 8, "dts", 8, "pts", 8, "sfl", 4)), stblw=dict(out_cap=("out", 1)),
               csub=dict(sub_cap=("sub", CR.SUBSAMPLE.itemsize)))[good.call]
    v.caps, v.room = dict(good.caps), dict(good.room)
    for cap, outs in per.items():
        more = ROOM_BYTES if outs[1] == 1 else ROOM_ITEMS
        v.caps[cap] += more
        for name, width in zip(outs[::2], outs[1::2]):
            v.room[name] += more * width
            v.spare[name] = more * width
    if good.call == "rtpo":
        v.a = dict(good.a, prm=dict(good.a["prm"], max_span=2 * case("rtpo", "large").a["prm"]["max_span"] + RTPO_BLOCK + 1))
    return v


def variant(good, what):
    key = (id(good), what)
    if key not in _cases:
        if what == "roomy":
            _cases[key] = roomy(good)
        else:
            _cases[key] = short(good, what) if what.startswith("short") else malformed(good, what == "bad_late")
    return _cases[key]


def names_the_entry(call):
    """does the call's summary name the lowest entry in error?  The header gives reserved[0] = 1 + that entry to
    hbs_lenpref_to_annexb, hbs_ts_demux and hbs_ts_mux; hbs_annexb_to_lenpref leaves it 0, and hbs_au_insert's reserved[]
    counts what it inserted, so both are 0 under HBS_E_ARG."""
    if call in RTP_CALLS:                          # "reserved[0] = 1 + the lowest offending NAL", "... faulty packet", "... faulty entry"
        return True
    # hbs_mp4_fragment: reserved[0] = 1 + the lowest offending NAL (and reserved[1] the AU); hbs_mp4_samples: reserved[0] the segment,
    # reserved[1] the moof, reserved[2] the sample; the two sample table calls name a box in reserved[0] and the sample in
    # reserved[2].  A malformed variant of these calls carries the word and the value the header promises it (Case.named)
    return call in ("l2a", "tsd", "tsm", "mp4f", "mp4s")


def writes_nothing_when_refused(call):
    """does the header promise that a call that reports an error writes nothing but the summary?  hbs_rtp_pack: "On either error
    nothing is written but the summary"; hbs_rtp_unpack: "On either error nothing but the summary is written"; hbs_rtp_order: "On
    any error nothing but the summary is written"; hbs_mp4_fragment and hbs_mp4_samples: "On any error nothing but the summary is
    written"; hbs_mp4_stbl_samples: "on any error only the summary is written"; hbs_mp4_stbl_write: "On any error nothing but the
    summary is written"; hbs_au_times: "the summary's error is HBS_E_DEPTH, ... and nothing but the summary is written";
    hbs_cenc_subsamples: "On an error only the summary is written"; hbs_cenc_crypt: "nothing but the summary is written", and
    hbs_cbcs_crypt has its checks (the buffer the crypt calls work in is no output in this sense: it holds what was uploaded, and
    is compared with that)."""
    return call in CALLS2 or call in CALLS3


def sequence(call, seed=1, B=188):
    """the ten steps of the sequence on one context -> [(case, plan only?)]"""
    small, large, odd = (case(call, w, seed, B) for w in SIZES)
    return [(large, False), (small, False), (variant(large, "bad_late"), False), (small, False), (variant(small, "bad_early"), False),
            (odd, False), (empty(call, B), False), (variant(large, "short"), False), (large, True), (large, False)]


def sequence2(call, seed=1):
    """the steps of a CALLS2 sequence on one context: the ten steps, a roomy call behind the first large one and behind the short
    ones, and a step for each capacity a byte or an entry short -> [(case, plan only?)]"""
    small, large, odd = (case(call, w, seed) for w in SIZES)
    steps = [(large, False), (variant(large, "roomy"), False), (small, False), (variant(large, "bad_late"), False), (small, False),
             (variant(small, "bad_early"), False), (odd, False), (empty(call), False)]
    steps += [(variant(large, what), False) for what in SHORTS[call]]
    return steps + [(variant(small, "roomy"), False), (large, True), (large, False)]


# ---- the timing and encryption calls (CALLS3) ------------------------------------------------------------------------------------
# A case of hbs_au_times holds the AU table, the keywords of T.params_record and the tables it asks for (`outs`); one of
# hbs_cenc_subsamples the stream, the index and the AU numbers with d_keep / d_payload_off or None; one of the crypt calls the
# data, the four tables, the key, either the per-sample IVs (`iv`) or the constant / first one (`iv0`), for hbs_cenc_crypt whether
# a d_iv receives the counter blocks (`ivo`), for hbs_cbcs_crypt the pattern.  The three crypt calls take one set of tables a
# size; the data buffer is their output: a step uploads it fresh and compares all of it.

def crypt_entries(a):
    return int(a["first"][-1]) if len(a["off"]) else 0


def reference3(case, plan):
    a, c = case.a, ({} if plan else case.caps)
    if case.call == "aut":                         # (a plan has all four tables NULL and writes the summary alone)
        r = T.au_times(a["au"], **a["kw"])
        return tuple(None if plan else r[name] for name, _ in AUT_TABLES) + (r["summary"],)
    if case.call == "csub":                        # (a plan writes d_sub_first; under HBS_E_ARG "the counts mean nothing")
        idx = a["index"]
        r = CR.subsamples(a["stream"], idx["start"].astype(np.int64), idx["end"].astype(np.int64), a["nal_au"], a["n_aus"], a["L"], keep=a["keep"],
                          payload_off=a["po"], flags=a["flags"], clear_lead=a["clear_lead"], sub_cap=c.get("sub_cap"))
        if r["error"] == E_ARG:
            return None, None, dict(error=E_ARG, nal_found=len(idx), stop_reason=0, reserved=[r["bad"], 0, None])
        s = dict(error=r["error"], nal_count=len(r["sub"]), nal_found=len(idx), rbsp_bytes=r["protected"], stream_bytes=r["sample_bytes"],
                 stop_reason=0, reserved=[0, 0, r["kept"]])
        return (r["sub_first"] if not r["error"] else None), (r["sub"] if not r["error"] and not plan else None), s
    n, cenc = len(a["off"]), case.call == "cenc"
    s = dict(error=0, nal_count=crypt_entries(a), nal_found=n, rbsp_bytes=0, stream_bytes=len(a["data"]), stop_reason=0, reserved=[0, 0, 0])
    bad = CR.crypt_check(len(a["data"]), a["off"], a["size"], a["first"], a["sub"]) if n else 0
    if bad:                                        # counts 0, the data as it was
        s.update(error=E_ARG, nal_count=0, reserved=[bad, 0, 0])
        return (a["data"],) + ((None,) if cenc else ()) + (s,)
    if cenc:
        out, s["rbsp_bytes"], used = CR.crypt(a["data"], a["off"], a["size"], a["first"], a["sub"], a["key"], iv=a["iv"], iv0=a["iv0"])
        return out, (used.reshape(-1) if a["ivo"] else None), s
    out, s["rbsp_bytes"] = CB.crypt_many(a["data"], a["off"], a["size"], a["first"], a["sub"], a["key"], iv=a["iv"], iv0=a["iv0"], c=a["c"], k=a["k"],
                                         whole=a["whole"], decrypt=case.call == "cbcsd")
    return out, s


def needs3(case):
    a = case.a
    if case.call == "aut":                         # no capacity: each table it asks for has n_aus entries
        return {}, {name: len(a["au"]) * width for name, width in AUT_TABLES if name in a["outs"]}
    if case.call == "csub":
        s = want(case, plan=True)[-1]
        assert s["error"] == 0, (case, s)
        return dict(sub_cap=s["nal_count"]), dict(sf=(a["n_aus"] + 1) * 8, sub=s["nal_count"] * CR.SUBSAMPLE.itemsize)
    return {}, dict(data=len(a["data"]), **(dict(ivo=16 * len(a["off"])) if a.get("ivo") else {}))


def make_aut(which, seed):
    """small: pyramids, two heads, AUs without a picture.  large: six workgroups, the last ragged; heads on the last AU of workgroup
    0 and the first of workgroup 1; AUs without a picture across the edge of workgroups 1 and 2; the last AU of workgroup 2 has a
    key above those of the 80 and more AUs behind it (its forward walk leaves the halo), and 80 AUs in front of the first AU of
    workgroup 4 lies a key above that AU's (its backward walk does).  odd: HBS_AUT_WRAP33 across 2^33, a delay given below R, and
    only d_pts and d_display asked for"""
    rng = np.random.default_rng(seed + 1100)
    B, outs = AUT_BLOCK, tuple(name for name, _ in AUT_TABLES)
    if which == "small":
        n = 200
        au, kw = T.table(T.pyramid(8, n // 8 + 1)[:n], heads=[64, 130], nopic=[5, 70, 71], junk=rng), dict(tick=3003, base_time=90000)
    elif which == "odd":
        n = B + 100
        au = T.table(T.pyramid(16, n // 16 + 1)[:n], heads=[B + 1], junk=rng)
        R = T.au_times(au)["summary"]["reserved"][1]
        kw, outs = dict(tick=3003, base_time=(1 << 33) - 3003 * 5 - 1, flags=T.WRAP33, delay=R - 2), ("pts", "display")
    else:
        n = 5 * B + 11
        keys = 4 * np.asarray(T.pyramid(8, n // 8 + 1)[:n], dtype=np.int64)
        keys[3 * B - 1] = 4 * (3 * B - 1 + 85)
        keys[4 * B - 80] = 4 * (4 * B + 12)
        au = T.table(keys.tolist(), heads=[B - 1, B], nopic=list(range(2 * B - 3, 2 * B + 4)), junk=rng)
        kw = dict(tick=3003, base_time=90000)
    return finish(Case("aut", which, dict(au=au, kw=kw, outs=outs)))


def cenc_stream(rng, n_nals, n_aus, L, keep, po, edges=(), big=False):
    """n_nals small NALs of types 1, 19, 32..34, 39, 35 behind 3-byte gaps in n_aus AUs, two of them with nothing kept; at every NAL
    of `edges` four kept parameter sets of one AU, two on either side; with `big` a 70 000-byte SEI in front of a slice of its AU
    (a clear run above 65 535) and an SEI that is alone in its AU and, with its four length bytes, 2 x 65 535 bytes long
    -> (stream, index, nal_au, keep or None, payload_off or None)"""
    types = rng.choice([1, 19, 32, 33, 34, 39, 35], n_nals)
    sizes = rng.integers(0, 90 if L > 1 else 60, n_nals)
    kept = (rng.integers(0, 5, n_nals) > 0).astype(np.uint8) if keep else np.ones(n_nals, dtype=np.uint8)
    same, alone = {51} if big else set(), [200] if big else []          # NALs that continue their AU; NALs that are an AU
    for e in edges:
        types[e - 2:e + 2], sizes[e - 2:e + 2], kept[e - 2:e + 2] = 33, 20, 1
        same |= {e - 1, e, e + 1}
    if big:
        assert L == 4
        types[50], sizes[50], kept[50] = 39, 70000, 1
        types[51], sizes[51], kept[51] = 1, 50, 1
        types[200], sizes[200], kept[200] = 39, 2 * CR.MAX_CLEAR - L, 1
    rises = {k for a in alone for k in (a, a + 1)}
    free = [k for k in range(1, n_nals) if k not in same and k not in rises]
    inc = np.zeros(n_nals, dtype=np.uint32)
    inc[sorted(rises) + rng.permutation(free)[: n_aus - 1 - len(rises)].tolist()] = 1
    nal_au = (np.cumsum(inc) + 3).astype(np.uint32)
    sizes[(types < 32) & (sizes == 1)] = 2
    if keep:
        for a in (nal_au[30], nal_au[120]):
            kept[nal_au == a] = 0
    starts = np.cumsum(sizes + 3) - sizes
    ends = starts + sizes
    stream = rng.integers(0, 256, int(ends[-1]) + 9, dtype=np.uint8)
    at = starts[sizes > 0]
    stream[at] = (types[sizes > 0] << 1).astype(np.uint8) | (stream[at] & 0x81)
    off = np.full(n_nals, CR.M64, dtype=np.uint64)
    vcl = np.flatnonzero((types < 32) & (sizes >= 2))
    off[vcl] = (starts[vcl] + rng.integers(2, sizes[vcl] + 1)).astype(np.uint64)
    index = np.zeros(n_nals, dtype=F.NAL_ENTRY)
    index["start"], index["end"] = starts, ends
    return stream, index, nal_au, (kept if keep else None), (off if po else None)


# NALs of the hbs_cenc_subsamples cases: one plan workgroup; two and a ragged third with AUs and clear runs across both edges and
# the long clear runs; between them with 1-byte lengths, no d_keep, no d_payload_off, HBS_CENC_ALIGN16 and a clear lead of 2
CSUB = dict(small=dict(n=400, aus=200, L=4, keep=True, po=True, flags=0, lead=96, edges=(), big=False),
            large=dict(n=2 * CENC_NAL_BLOCK + 900, aus=1700, L=4, keep=True, po=True, flags=0, lead=96, edges=(CENC_NAL_BLOCK, 2 * CENC_NAL_BLOCK), big=True),
            odd=dict(n=CENC_NAL_BLOCK + 500, aus=900, L=1, keep=False, po=False, flags=CR.ALIGN16, lead=2, edges=(), big=False))


def make_csub(which, seed):
    p = CSUB[which]
    stream, index, nal_au, keep, po = cenc_stream(np.random.default_rng(seed + 1200), p["n"], p["aus"], p["L"], p["keep"], p["po"], p["edges"], p["big"])
    return finish(Case("csub", which, dict(stream=stream, index=index, nal_au=nal_au, n_aus=p["aus"], keep=keep, po=po, L=p["L"], flags=p["flags"],
                                           clear_lead=p["lead"])))


def crypt_tables(which, seed):
    """the data and the four tables of one size, shared by the three crypt calls (built once).  Samples at odd addresses with gaps
    of 1 to 9 bytes.  small: 120 samples of one to four entries.  large: 3 x 256 + 40 samples cut at random entries of 16 x 1 024 +
    300, half of them with 64 to 70 whole blocks and 0 to 15 bytes protected, the rest with 0 to 48 bytes.  odd: 356 samples of which
    four in ten have no entry and size 0, the first and the last among them.  hollow: 300 samples, none with an entry"""
    key = ("crypt tables", which, seed)
    if key in _cases:
        return _cases[key]
    rng = np.random.default_rng(seed + 1300)
    if which == "large":
        ns, E = 3 * CRYPT_SAMPLE_BLOCK + 40, 16 * CRYPT_RANGES + 300
        first = np.concatenate([[0], np.sort(rng.choice(np.arange(1, E), size=ns - 1, replace=False)), [E]])
        long_ = rng.random(E) < 0.5
        protect = np.where(long_, 16 * rng.integers(CBCS_LANE_BLOCKS, CBCS_LANE_BLOCKS + 7, E) + rng.integers(0, 16, E), rng.integers(0, 49, E))
    else:
        if which == "small":
            per = rng.integers(1, 5, 120)
        elif which == "odd":
            per = np.where(rng.random(CRYPT_SAMPLE_BLOCK + 100) < 0.4, 0, rng.integers(3, 12, CRYPT_SAMPLE_BLOCK + 100))
            per[[0, 7, 8, -1]] = 0
        else:
            per = np.zeros(300, dtype=np.int64)
        ns, E = len(per), int(per.sum())
        first = np.concatenate([[0], np.cumsum(per)])
        protect = rng.integers(0, 200, E)
    clear = rng.integers(0, 21, E)
    sub = np.zeros(E, dtype=CR.SUBSAMPLE)
    sub["clear"], sub["protect"] = clear, protect
    total = np.concatenate([[0], np.cumsum(clear + protect)])
    size = total[first[1:]] - total[first[:-1]]
    gaps = rng.integers(1, 10, ns)
    off = 3 + np.concatenate([[0], np.cumsum(size + gaps)[:-1]])
    data = rng.integers(0, 256, int(off[-1] + size[-1]) + CRYPT_TAIL, dtype=np.uint8)
    _cases[key] = dict(data=data, off=off.astype(np.uint64), size=size.astype(np.uint64), first=first.astype(np.uint64), sub=sub)
    return _cases[key]


def long_entries_a_range(a):
    """the entries of kCbcsLaneBlocks whole blocks and more in each of the 1 024 ranges (hbs_cenc.h: cenc_range_begin)"""
    E, G = crypt_entries(a), CRYPT_RANGES
    begin = [E // G * g + E % G * g // G for g in range(G + 1)]
    long_ = np.concatenate([[0], np.cumsum(a["sub"]["protect"] // 16 >= CBCS_LANE_BLOCKS)])
    return np.diff(long_[begin]), np.diff(begin)


def make_crypt(call):
    """small and large: the IVs of the samples in d_iv; hbs_cbcs_crypt 1:9 and 1:0 (every long entry of the large tables is
    kCbcsLaneBlocks crypt blocks or more).  odd and hollow: hbs_cenc_crypt with iv_mode 1 from ff..fe (the third sample's counter
    block wraps to 0) and a d_iv that receives the blocks; hbs_cbcs_crypt 3:7 with HBS_CBCS_WHOLE_RUNS, the constant IV, no d_iv"""
    def make(which, seed):
        t = crypt_tables(which, seed)
        rng = np.random.default_rng(seed + 1400 + CALLS3.index(call))
        plain = which in ("small", "large")
        a = dict(t, key=bytes(rng.integers(0, 256, 16, dtype=np.uint8)), iv=rng.integers(0, 256, 16 * len(t["off"]), dtype=np.uint8) if plain else None)
        if call == "cenc":
            a.update(iv0=None if plain else bytes.fromhex("fffffffffffffffe"), ivo=not plain)
        else:
            c, k = dict(small=(1, 9), large=(1, 0)).get(which, (3, 7))
            a.update(iv0=None if plain else bytes(rng.integers(0, 256, 16, dtype=np.uint8)), ivo=False, c=c, k=k, whole=not plain)
        return finish(Case(call, which, a))
    return make


MAKERS.update(aut=make_aut, csub=make_csub, cenc=make_crypt("cenc"), cbcs=make_crypt("cbcs"), cbcsd=make_crypt("cbcsd"))


def hollow(call, seed=1):
    """the table of a crypt call in which every sample has no entries and size 0"""
    return case(call, "hollow", seed)


def empty3(call):
    if call == "aut":
        return dict(au=T.table([]), kw=dict(delay=9), outs=tuple(name for name, _ in AUT_TABLES))
    if call == "csub":
        return dict(stream=np.zeros(0, dtype=np.uint8), index=np.zeros(0, dtype=F.NAL_ENTRY), nal_au=np.zeros(0, dtype=np.uint32), n_aus=0, keep=None,
                    po=None, L=4, flags=0, clear_lead=96)
    z64 = np.zeros(0, dtype=np.uint64)
    a = dict(data=np.random.default_rng(5).integers(0, 256, 100, dtype=np.uint8), off=z64, size=z64, first=np.zeros(1, dtype=np.uint64),
             sub=np.zeros(0, dtype=CR.SUBSAMPLE), key=bytes(range(16)), iv=None, iv0=bytes(range(16, 24 if call == "cenc" else 32)), ivo=False)
    if call != "cenc":
        a.update(c=1, k=9, whole=False)
    return a


# the check group a malformed variant of a crypt call fails (early, late): the sums (d_sample_size[j] += 1), the first group
# (d_sub_first falls behind sample j), the second (a clear count of 65 536 in sample j's first entry)
CRYPT_FAULTS = dict(cenc=("sums", "falling"), cbcs=("clear", "sums"), cbcsd=("falling", "clear"))


def malformed3(good, late):
    """hbs_au_times: a table with a span of HBS_AUT_MAX_SPAN + 1, tests/test_gpu_au_times.py::span_tables, with the good case's
    parameters and tables.  Both ends of such a span offend -- fwd of the AU in front, back of the AU behind -- so the lowest
    offending AU is always the one in front: `early` has it in the first workgroup, and `late` has the AU behind in the last
    workgroup, 1 025 AUs behind the one the summary names (no table can name an AU of its last workgroup).  hbs_cenc_subsamples:
    tests/test_gpu_cenc.py::test_a_slice_the_parse_did_not_read_is_an_error, "start+1".  The crypt calls: CRYPT_FAULTS, as
    test_each_error_alone of their modules"""
    a = dict(good.a)
    named_error = E_ARG
    if good.call == "aut":
        span, lead, tail = T.MAX_SPAN + 1, (45, 5) if late else (10, 40), None
        a["au"] = T.table([0] * lead[0] + [9] + [1] * span + [50] * lead[1], junk=np.random.default_rng(len(good.a["au"]) + late))
        at, among, named_error = lead[0], (len(a["au"]), AUT_BLOCK), E_DEPTH
    elif good.call == "csub":
        assert a["po"] is not None, "the fault is a d_payload_off"
        n, per = items(good)[0]
        at = 5 if not late else max((blocks(n, per) - 1) * per, n - 40)
        usable = (a["po"] != CR.M64) & (a["keep"] != 0 if a["keep"] is not None else True)
        at = at + int(np.flatnonzero(usable[at:])[0])          # the next kept VCL NAL of two bytes and more
        a["po"] = a["po"].copy()
        a["po"][at] = a["index"]["start"][at] + np.uint64(1)
        among = (n, per)
    else:
        n, per = items(good)[0]
        fault = CRYPT_FAULTS[good.call][1 if late else 0]
        at = max(n - 3, (blocks(n, per) - 1) * per) if late else min(5, n - 1)
        first = a["first"].astype(np.int64)
        if fault == "sums":                        # (a gap of a byte and more lies behind every sample, and CRYPT_TAIL behind the last)
            a["size"] = a["size"].copy()
            a["size"][at] += np.uint64(1)
        elif fault == "falling":
            at += int(np.flatnonzero(first[at:-1] > 0)[0])
            a["first"] = a["first"].copy()
            a["first"][at + 1] = a["first"][at] - np.uint64(1)
        else:
            at += int(np.flatnonzero(first[at + 1:] > first[at:-1])[0])          # the next sample with an entry
            e, more = int(first[at]), 65536 - int(a["sub"]["clear"][int(first[at])])
            a["sub"], a["size"], a["off"] = a["sub"].copy(), a["size"].copy(), a["off"].copy()
            a["sub"]["clear"][e] = 65536
            a["size"][at] += np.uint64(more)
            a["off"][at + 1:] += np.uint64(more)
            a["data"] = np.concatenate([a["data"], np.zeros(more, dtype=np.uint8)])
        among = (n, per)
    v = Case(good.call, good.name + (" bad-late" if late else " bad-early"), a, bad=at)
    v.caps, v.room = needs3(v) if good.call != "csub" else (dict(good.caps), dict(good.room))
    v.named, v.among, v.error = (0, at + 1), among, named_error
    return v


def sequence3(call, seed=1):
    """the steps of a CALLS3 sequence on one context: the ten steps; the crypt calls have the table without any entry behind the
    odd one and, having no plan, no plan-only step; hbs_cenc_subsamples alone has a capacity, so it alone has the step that is an
    entry short and the roomy one -> [(case, plan only?)]"""
    small, large, odd = (case(call, w, seed) for w in SIZES)
    steps = [(large, False), (small, False), (variant(large, "bad_late"), False), (small, False), (variant(small, "bad_early"), False), (odd, False)]
    if call in CRYPT_CALLS:
        steps.append((hollow(call, seed), False))
    steps.append((empty(call), False))
    if call == "csub":
        steps += [(variant(large, "short"), False), (variant(small, "roomy"), False)]
    if call not in CRYPT_CALLS:
        steps.append((large, True))
    return steps + [(large, False)]


# what the three crypt calls do one after the other in the one buffer they share: (call, case)
SHARED_CRYPT = (("cenc", "large"), ("cbcsd", "small"), ("cbcs", "large"), ("cenc", "small"), ("cbcsd", "large"), ("cenc", "hollow"), ("cbcsd", "small"),
                ("cbcs", "large bad-late"), ("cenc", "small"), ("cbcsd", "odd"), ("cbcsd", "hollow"), ("cenc", "large"))


def shared_crypt_steps(seed=1):
    out = []
    for call, name in SHARED_CRYPT:
        which, _, bad = name.partition(" ")
        c = case(call, which, seed)
        out.append((variant(c, bad.replace("-", "_")) if bad else c, False))
    return out
