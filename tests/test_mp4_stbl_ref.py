"""The Python reference of hbs_mp4_stbl_samples / hbs_mp4_stbl_find_host (tests/_mp4_stbl_ref.py): its writer and its reader,
which share nothing but the box writer, agree on random tracks; and the reader gives the tables computed by hand for one small
file that is committed here as hex."""
import numpy as np
import pytest

from tests import _mp4_stbl_ref as S
from tests.test_mp4_read_ref import NALS

# ftyp, moov, mdat.  Five samples of 5, 6, 7, 5, 6 bytes in three chunks (2, 2, 1 samples: a stsc of the two entries (1, 2) and
# (3, 1)) that lie back to back from byte 828 on; stts (3 x 100, 2 x 50); ctts version 1: 200, -50, 100, 0, 50; stss: 1, 4.
FIXED = bytes.fromhex(
    "000000186674797069736f360000000069736f366d7034310000031c6d6f6f760000006c6d76686400000000000000000000000000015f9000000000"
    "000100000100000000000000000000000001000000000000000000000000000000010000000000000000000000000000400000000000000000000000"
    "0000000000000000000000000000000000000002000002a87472616b0000005c746b6864000000030000000000000000000000010000000000000000"
    "000000000000000000000000000000000001000000000000000000000000000000010000000000000000000000000000400000000780000004380000"
    "000002446d646961000000206d64686400000000000000000000000000015f900000000055c400000000002d68646c72000000000000000076696465"
    "000000000000000000000000566964656f48616e646c657200000001ef6d696e6600000014766d68640000000100000000000000000000002464696e"
    "660000001c6472656600000000000000010000000c75726c2000000001000001af7374626c000000cb737473640000000000000001000000bb687663"
    "310000000000000001000000000000000000000000000000000780043800480000004800000000000000010000000000000000000000000000000000"
    "0000000000000000000000000000000018ffff00000065687663430101600102030405060708090af000fcfdf8f800000f03a00001001240010c01ff"
    "ff016000000000000000000000a10001001842010101600102030405060708090a0b0c0d0e0f10111213a2000200054401c172b400064401c0f7c0cc"
    "00000020737474730000000000000002000000030000006400000002000000320000003863747473010000000000000500000001000000c800000001"
    "ffffffce0000000100000064000000010000000000000001000000320000001873747373000000000000000200000001000000040000002873747363"
    "0000000000000002000000010000000200000001000000030000000100000001000000287374737a0000000000000000000000050000000500000006"
    "0000000700000005000000060000001c7374636f00000000000000030000033c0000034700000353000000256d646174000000014100000002424200"
    "0000034343430000000144000000024545")
FIXED_OFF = [828, 833, 839, 846, 851]
FIXED_SIZE = [5, 6, 7, 5, 6]
FIXED_DTS = [0, 100, 200, 300, 350]
FIXED_PTS = [200, 50, 300, 300, 400]
FIXED_FLAGS = [0, 0x10000, 0x10000, 0, 0x10000]


def test_fixed_file_by_hand():
    rec = S.find(FIXED)
    # the payloads lie where a hex dump shows them: stts, ctts, stss, stsc, stsz, stco in file order
    assert [tuple(int(x) for x in rec[n][0]) for n in S.BOXES] == [(760, 32), (800, 20), (720, 32), (608, 24), (640, 48), (696, 16)]
    assert int(rec["flags"][0]) == 0 and int(rec["file_bytes"][0]) == 0
    assert FIXED[640] == 1 and FIXED[660:664] == b"\xff\xff\xff\xce"          # ctts version 1, the second offset -50
    assert FIXED[720 + 4:720 + 8] == b"\x00\x00\x00\x02" and FIXED[696 + 4:696 + 8] == b"\x00\x00\x00\x02"   # stsc and stss of 2
    off, size, dts, pts, flags, s = S.read(FIXED, rec)
    assert s == S.summary(0, 5, 3, 29, len(FIXED))
    assert (off.tolist(), size.tolist(), dts.tolist(), pts.tolist(), flags.tolist()) == (FIXED_OFF, FIXED_SIZE, FIXED_DTS, FIXED_PTS, FIXED_FLAGS)
    assert [FIXED[o + 4:o + n] for o, n in zip(FIXED_OFF, FIXED_SIZE)] == [b"A", b"BB", b"CCC", b"D", b"EE"]
    # a moov cut out of the file, with its position as the base, gives the same record
    at = FIXED.index(b"moov") - 4
    size_moov = int.from_bytes(FIXED[at:at + 4], "big")
    assert S.find(FIXED[at:at + size_moov], base=at).tobytes() == rec.tobytes()
    assert S.read(FIXED, rec, outputs=False)[5] == s and S.read(FIXED, rec, sample_cap=4)[5] == S.summary(S.E_CAPACITY, 5, 3, 0, len(FIXED))


@pytest.mark.parametrize("seed", range(8))
def test_writer_and_reader_agree_on_random_tracks(seed):
    rng = np.random.default_rng(4000 + seed)
    n = int(rng.integers(0, 120))
    co64, constant, moov_first = bool(seed & 1), (9 if seed == 3 else None), seed % 3 != 2
    t = S.random_track(rng, n, reorder=seed % 4 != 1, constant=constant)
    sync = None if seed == 5 else t["sync"]
    data, offs = S.progressive_file(t["samples"], t["chunk_lens"], t["deltas"], t["cts"], sync, nals=NALS, co64=co64, constant=constant,
                                    moov_first=moov_first, gaps=seed % 3)
    rec = S.find(data, track_id=seed % 2)
    assert bool(int(rec["flags"][0]) & S.CO64) == co64
    off, size, dts, pts, flags, s = S.read(data, rec)
    assert s == S.summary(0, n, len(t["chunk_lens"]), sum(len(x) for x in t["samples"]), len(data))
    assert off.tolist() == offs and size.tolist() == [len(x) for x in t["samples"]]
    assert [data[o:o + len(x)] for o, x in zip(offs, t["samples"])] == t["samples"]
    want_dts = [sum(t["deltas"][:i]) for i in range(n)]
    assert dts.tolist() == want_dts
    assert pts.tolist() == [d + c for d, c in zip(want_dts, t["cts"] or [0] * n)]
    assert flags.tolist() == [0 if sync is None or i in sync else S.NON_SYNC for i in range(n)]


def test_reader_reports_errors_at_their_box_and_sample():
    sizes, lens, offs, deltas = [4, 5, 6, 7], [3, 1], [100, 200], [10, 10, 10, 10]
    pay = S.payloads(sizes, lens, offs, deltas, cts=[0, 5, 0, 0], sync=[0, 2])

    def err(change, **kw):
        p = dict(pay)
        p.update(change)
        buf, rec = S.layout(p)
        rec["file_bytes"] = kw.pop("file_bytes", 1000)
        return S.read(buf, rec, **kw)[5]

    assert err({})["error"] == 0
    assert err({"stsz": S.p_stsz(sizes, count=5)})["reserved"] == [1, 0, 0]
    assert err({"stco": S.p_stco(offs, version=1)})["reserved"] == [2, 0, 0]
    assert err({"stsc": S.p_stsc([(1, 3), (1, 1)])})["reserved"] == [3, 0, 0]
    assert err({"stsc": S.p_stsc([(1, 3), (3, 1)])})["reserved"] == [3, 0, 0]
    assert err({"stsc": S.p_stsc([(1, 1)])})["reserved"] == [3, 0, 0]                  # the chunks hold 2 samples
    assert err({"stsc": S.p_stsc([(1, 0), (2, 4)])})["error"] == 0
    assert err({"stts": S.p_pairs([(3, 10)])})["reserved"] == [4, 0, 0]
    assert err({"ctts": S.p_pairs([(1, 0)], version=2)})["reserved"] == [5, 0, 0]
    assert err({"stss": S.p_stss([2, 2])})["reserved"] == [6, 0, 0]
    assert err({"stss": S.p_stss([0])})["reserved"] == [6, 0, 0]
    assert err({"stss": S.p_stss([1, 9])})["error"] == 0
    assert err({"stts": S.p_pairs([(3, 10)]), "stss": S.p_stss([0])})["reserved"] == [4, 0, 0]
    assert err({}, file_bytes=114)["reserved"] == [0, 0, 3]
    assert err({"stts": S.p_pairs([(2, 1 << 31), (2, (1 << 32) - 1)]), "ctts": None})["error"] == 0
    assert err({"ctts": S.p_pairs([(2, 0), (1, -21)], version=1, signed=True)})["reserved"] == [0, 0, 3]
    assert err({"ctts": S.p_pairs([(2, 0), (1, -20)], version=1, signed=True)})["error"] == 0
