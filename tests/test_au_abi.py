"""hbs_access_units / hbs_au_keep on the CPU side: symbols, record layouts, flag values, and the sequential reference
(tests/_au_ref.py) on hand-written cases whose answers are worked out here from H.265 7.4.2.4.4 and 8.3.1."""
import os
import re

import numpy as np

from tests import _au_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF = 40


def run(nals, carry=None):
    index, parsed, compact, structs = R.fabricate(nals, OFF)
    return R.access_units(index, parsed, compact, structs, OFF, carry)


def V(t, first=1, lsb=0, tid1=1, **kw):
    return dict(type=t, first=first, lsb=lsb, tid1=tid1, **kw)


def N(t, **kw):
    return dict(type=t, **kw)


def test_symbols_declared_and_exported():
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import EXPORTS
    from tests.test_abi_exports import declared_functions
    lib = hbs.load_library()
    for name in ("hbs_access_units", "hbs_au_keep", "hbs_au_sps_poc_offset"):
        assert name in declared_functions(), name
        assert name in EXPORTS, name
        assert hasattr(lib, name), name
    off = int(lib.hbs_au_sps_poc_offset())
    assert 0 < off < int(lib.hbs_sps_tables_offset()) and off % 4 == 0


def test_records_and_flags():
    import hevcbitstream_amd as hbs
    assert hbs.ACCESS_UNIT.itemsize == 64 and hbs.AU_CARRY.itemsize == 16
    assert [hbs.ACCESS_UNIT.fields[f][1] for f in hbs.ACCESS_UNIT.names] == [0, 8, 16, 24, 28, 32, 36, 40, 44, 48, 52, 56, 60]
    assert [hbs.AU_CARRY.fields[f][1] for f in hbs.AU_CARRY.names] == [0, 4, 8, 12]
    hdr = open(os.path.join(ROOT, "include", "hevcbitstream_amd.h")).read()
    for name, val in (("IRAP", hbs.AU_IRAP), ("IDR", hbs.AU_IDR), ("CVS_START", hbs.AU_CVS_START), ("ANCHOR", hbs.AU_ANCHOR),
                      ("NO_PICTURE", hbs.AU_NO_PICTURE), ("DAMAGED", hbs.AU_DAMAGED), ("PARAM_SETS", hbs.AU_PARAM_SETS),
                      ("END_OF_SEQ", hbs.AU_END_OF_SEQ)):
        m = re.search(r"#define HBS_AU_%s\s+(\d+)" % name, hdr)
        assert m and int(m.group(1)) == val, name
        assert getattr(R, name) == val
    assert [1 << i for i in range(8)] == [hbs.AU_IRAP, hbs.AU_IDR, hbs.AU_CVS_START, hbs.AU_ANCHOR, hbs.AU_NO_PICTURE, hbs.AU_DAMAGED,
                                          hbs.AU_PARAM_SETS, hbs.AU_END_OF_SEQ]
    m = re.search(r"#define HBS_AUKEEP_PARAM_SETS\s+(\d+)", hdr)
    assert m and int(m.group(1)) == hbs.AUKEEP_PARAM_SETS == 1


def test_non_vcl_nals_in_front_join_the_picture_behind_them():
    # AUD VPS SPS PPS SEI | IDR (2 segments) suffix-SEI EOS | AUD prefix-SEI TRAIL suffix-SEI | TRAIL | TRAIL
    nals = [N(35), N(32), N(33, log2=0), N(34), N(39), V(19), V(19, first=0), N(40), N(36),
            N(35), N(39), V(1, lsb=1), N(40),
            V(1, lsb=2),
            V(1, lsb=3), V(1, first=0, lsb=3, dep=1, stype=1)]
    au, nal_au, carry, s = run(nals)
    assert nal_au.tolist() == [0] * 9 + [1] * 4 + [2] + [3] * 2
    assert au["first_nal"].tolist() == [0, 9, 13, 14]
    assert au["nal_count"].tolist() == [9, 4, 1, 2] and au["vcl_count"].tolist() == [2, 1, 1, 2]
    assert au["first_vcl"].tolist() == [5, 2, 0, 0]
    assert au["unit_begin"].tolist() == [0, 90, 130, 140] and au["unit_end"].tolist() == [90, 130, 140, 160]
    assert au["nal_unit_type"].tolist() == [19, 1, 1, 1] and au["pic_order_cnt"].tolist() == [0, 1, 2, 3]
    assert int(au["flags"][0]) == R.IRAP | R.IDR | R.CVS_START | R.ANCHOR | R.PARAM_SETS | R.END_OF_SEQ
    assert au["flags"][1:].tolist() == [R.ANCHOR] * 3
    assert au["slice_types"].tolist() == [1, 1, 1, 1]          # the dependent segment's slice_type 1 does not count
    assert s == dict(nal_count=4, nal_found=16, pictures=4, cvs_starts=1, stream_bytes=160)
    assert int(carry["flags"][0]) == 3 and int(carry["anchor_poc_lsb"][0]) == 3 and int(carry["anchor_poc_msb"][0]) == 0


def test_second_candidate_behind_a_picture_does_not_start_again_and_other_layers_ride_along():
    # TRAIL | SPS PPS (layer-1 slice, layer-1 SPS) TRAIL (type -1) | filler + reserved 45 stay
    nals = [V(1), N(33), N(34), V(1, layer=1), N(33, layer=1), V(1, lsb=1), N(-1), N(38), N(45)]
    au, nal_au, _, s = run(nals)
    assert nal_au.tolist() == [0, 1, 1, 1, 1, 1, 1, 1, 1]
    assert au["vcl_count"].tolist() == [1, 1] and au["first_vcl"].tolist() == [0, 4]
    assert int(au["flags"][1]) == R.ANCHOR | R.PARAM_SETS | R.DAMAGED


def test_no_vcl_at_all_and_empty():
    au, nal_au, carry, s = run([N(32), N(33), N(39), N(35)])
    assert len(au) == 1 and int(au["flags"][0]) == R.NO_PICTURE | R.PARAM_SETS and int(au["first_vcl"][0]) == 0xFFFFFFFF
    assert int(au["nal_unit_type"][0]) == -1 and s["pictures"] == 0 and int(carry["flags"][0]) == 0
    au, nal_au, carry, s = run([])
    assert len(au) == 0 and s["nal_count"] == 0 and s["stream_bytes"] == 0


def test_damaged_rule():
    au, _, _, _ = run([V(19), N(39, rc=-1), N(36, rc=-1), V(1, lsb=1, rc=-1), V(1, lsb=2), N(34, rc=-1)])
    # IDR | SEI EOS TRAIL(failed) | TRAIL | PPS(failed): failed SEI / EOS parses are what read_hevc_nal_unit always reports
    assert [int(f) & R.DAMAGED for f in au["flags"]] == [0, R.DAMAGED, 0, R.DAMAGED]


def test_poc_wraps_with_4_and_8_bits():
    for log2, mx in ((0, 16), (4, 256)):
        step = mx // 2 - 1                                         # the largest step 8.3.1 follows, upwards six times, then down again
        pocs = [step * i for i in range(7)] + [step * (6 - i) for i in range(1, 6)]
        nals = [N(33, log2=log2), V(19)] + [V(1, lsb=p % mx) for p in pocs[1:]]
        au, _, carry, _ = run(nals)
        assert au["pic_order_cnt"].tolist() == pocs
        assert int(carry["anchor_poc_msb"][0]) == 0 and int(carry["anchor_poc_lsb"][0]) == step
    # without an SPS struct in front Max is 16; below zero the msb goes negative
    au, _, _, _ = run([V(21, lsb=2), V(1, lsb=14), V(1, lsb=3)])
    assert au["pic_order_cnt"].tolist() == [2, -2, 3]


def test_only_anchors_feed_the_msb():
    # Max 16.  IDR(0); lsb 12 as RASL / RADL / TSA_N / tid 2: none becomes prevTid0Pic, so lsb 2 behind each is POC 2, not 18
    for t, tid1 in ((8, 1), (6, 1), (2, 1), (0, 1), (1, 2), (21, 2)):
        au, _, _, _ = run([V(19), V(t, lsb=7, tid1=tid1), V(t, lsb=12, tid1=tid1), V(1, lsb=2)])
        assert au["pic_order_cnt"].tolist()[-1] == 2, t
        assert not int(au["flags"][1]) & R.ANCHOR
    au, _, _, _ = run([V(19), V(1, lsb=7), V(1, lsb=12), V(1, lsb=2)])
    assert au["pic_order_cnt"].tolist() == [0, 7, 12, 18]


def test_msb_resets():
    def pocs(nals, carry=None):
        au, _, c, s = run(nals, carry)
        return au["pic_order_cnt"].tolist(), [bool(int(f) & R.CVS_START) for f in au["flags"]], c
    up = [V(1, lsb=7), V(1, lsb=14), V(1, lsb=5)]                       # 7 14 21 behind a picture with POC 0
    assert pocs([V(19)] + up + [V(19)] + [V(1, lsb=3)])[0] == [0, 7, 14, 21, 0, 3]
    assert pocs([V(19)] + up + [V(17, lsb=9)] + [V(1, lsb=1)])[0] == [0, 7, 14, 21, 9, 17]      # BLA: msb 0, lsb kept
    p, c, _ = pocs([V(21, lsb=4)] + up + [V(21, lsb=9)] + [V(1, lsb=1)])                        # first CRA resets, mid-stream CRA does not
    assert p == [4, 7, 14, 21, 25, 33] and c == [True, False, False, False, False, False]
    p, c, _ = pocs([V(21, lsb=4)] + up + [N(36), N(35), V(21, lsb=9)] + [V(1, lsb=1)])          # CRA behind EOS
    assert p == [4, 7, 14, 21, 9, 17] and c == [True, False, False, False, True, False]
    # the carry: a continuing batch's first CRA is a mid-stream CRA, unless an EOS is pending
    _, _, carry = pocs([V(21, lsb=4)] + up)
    assert int(carry["flags"][0]) == 3 and int(carry["anchor_poc_lsb"][0]) == 5 and int(carry["anchor_poc_msb"][0]) == 16
    assert pocs([V(21, lsb=9), V(1, lsb=1)], carry)[0] == [25, 33]
    _, _, carry = pocs([V(21, lsb=4)] + up + [N(36)])
    assert int(carry["flags"][0]) == 7
    assert pocs([V(21, lsb=9), V(1, lsb=1)], carry)[0] == [9, 17]


def test_hierarchical_b_gop():
    order = [8, 4, 2, 1, 3, 6, 5, 7]
    tid = {8: 1, 4: 2, 2: 3, 6: 3, 1: 4, 3: 4, 5: 4, 7: 4}
    for scale, log2 in ((1, 0), (2, 4)):
        nals = [N(32), N(33, log2=log2), N(34), V(19)]
        for gop in range(5):
            for o in order:
                nals += [N(35), V(1 if tid[o] == 1 else 0 if tid[o] == 4 else 1, lsb=(scale * (8 * gop + o)) % (16 << log2), tid1=tid[o]),
                         V(1, first=0)]
        au, _, _, s = run(nals)
        assert s["pictures"] == 41 and len(au) == 41
        assert sorted(au["pic_order_cnt"].tolist()) == [scale * i for i in range(41)]
        assert au["nal_count"].tolist() == [4] + [3] * 40


def test_au_keep_reference():
    nals = [N(32), N(33), N(34), V(19), V(1, lsb=1), N(34, rc=-1), N(34), V(1, lsb=2), N(33), V(1, lsb=3)]
    index, parsed, compact, structs = R.fabricate(nals, OFF)
    _, nal_au, _, _ = R.access_units(index, parsed, compact, structs, OFF)
    assert nal_au.tolist() == [0, 0, 0, 0, 1, 2, 2, 2, 3, 3]
    assert R.au_keep(nal_au, parsed, 2, 1, False).tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 0, 0]
    assert R.au_keep(nal_au, parsed, 2, 1, True).tolist() == [1, 1, 1, 0, 0, 1, 1, 1, 0, 0]
    assert R.au_keep(nal_au, parsed, 3, 9, True).tolist() == [1, 1, 0, 0, 0, 0, 1, 0, 1, 1]       # the failed PPS is passed over, the SPS inside the range is not "in front"; clipped
    assert R.au_keep(nal_au, parsed, 4, 2, True).tolist() == [0] * 10 and R.au_keep(nal_au, parsed, 1, 0, True).tolist() == [0] * 10


def test_generator_poc_override_leaves_other_draws_alone():
    from tests.hevc_synth import Synth
    a, b = Synth(5, rich=False), Synth(5, rich=False)
    for g in (a, b):
        g.vps(); g.sps_nal(1920, 1080); g.pps_nal()
    x = a.slice_nal(1, payload=b"\x11" * 8)
    y = b.slice_nal(1, payload=b"\x11" * 8, poc_lsb=3)
    assert x != y or a.sps["poc_bits"] == 0      # (the lengths may differ by an emulation prevention byte)
    assert a.slice_nal(1, payload=b"\x22" * 8) == b.slice_nal(1, payload=b"\x22" * 8)     # the random state went the same way
