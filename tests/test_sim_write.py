"""The syntax writers (write_hevc_nal_unit, hevc_stream.c:1249-1327) single-stepped on the CPU against
golden outputs of the reference's writer on parsed and on edited structs (tests/golden/make_golden_write.py)."""
import gzip
import json
import os

import numpy as np

from tests import _orc, _sim
from tests._parsecmp import which_struct
from tests.hevc_synth import annexb

from tests._writegold import field_index, slot_bytes

HERE = os.path.dirname(os.path.abspath(__file__))


def run_sequence(orc, steps):
    nals = [bytes.fromhex(s["nal"]) for s in steps]
    stream = np.frombuffer(annexb(nals), dtype=np.uint8)
    idx, arena, _ = _sim.index_extract(stream)
    assert len(idx) == len(nals)
    parsed, structs = _sim.parse_headers(arena, idx)
    last = {"sps": None, "pps": None}
    for k, st in enumerate(steps):
        t = int(parsed["nal_unit_type"][k])
        kind = which_struct(t)
        assert int(parsed["rc"][k]) == st["read_rc"], k
        if "write_rc" in st:
            off = int(parsed["struct_off"][k])
            slot = structs[off:off + slot_bytes(kind)].copy()
            view = slot.view(np.int32)
            for name, value in st["edits"]:
                view[field_index(kind, name)] = value
            cap = st["size"] * 3 // 4
            res, region = _sim.write_nal(t, int(parsed["nal_layer_id"][k]), int(parsed["nal_temporal_id_plus1"][k]), slot,
                                         last["sps"], last["pps"], cap, whole=True)
            rbsp = region[:int(res["rbsp_size"])]
            # behind rbsp_size the buffer stays as cleared: an SPS ends on an unfinished byte, whose bits are not part of the result
            assert not region[int(res["rbsp_size"]):].any(), (k, kind)
            if st["write_rc"] < 0:
                assert int(res["rc"]) < 0, k
            else:
                assert int(res["rc"]) == 0, (k, kind)
                rc, _, out = orc.rbsp_to_nal(bytes(rbsp))
                assert rc == st["write_rc"] and out.hex() == st["out"], (k, kind, st["edits"], out.hex()[:80], st["out"][:80])
                if kind == "sh":
                    assert int(res["slice_data_size"]) == st["slice_data_size"], k
        # parameter sets in force for later NALs: the stream's own (the golden script undoes its edits)
        if kind in ("sps", "pps") and int(parsed["rc"][k]) >= 0:
            off = int(parsed["struct_off"][k])
            last[kind] = structs[off:off + slot_bytes(kind)].copy()


def test_writers_match_reference(orc):
    vectors = json.load(gzip.open(os.path.join(HERE, "golden", "write_vectors.json.gz"), "rt"))
    assert len(vectors) >= 8
    for v in vectors:
        run_sequence(orc, v["steps"])


def test_sequences_parse_the_same_in_one_batch():
    """What tests/test_gpu_write.py builds on when it holds every NAL of a batch of all ten sequences (tiled: the ten again
    behind themselves, W.TILES times) against what the reference wrote for the sequence alone: parsed as one stream, every step keeps
    the rc and the struct (an SPS: with its derived tables) it has when its sequence is parsed by itself."""
    from tests import _writegold as W
    seqs = W.vectors()
    alone = []
    for v in seqs:
        g = W.Gold([v])
        idx, arena, _ = _sim.index_extract(np.frombuffer(annexb(g.nals), dtype=np.uint8))
        parsed, structs = _sim.parse_headers(arena, idx, fix=1)
        assert np.array_equal(parsed["rc"], g.read_rc), v["seed"]
        for k in range(g.n):
            off = int(parsed["struct_off"][k])
            alone.append((v["seed"], k, int(parsed["rc"][k]), g.kind[k], structs[off:off + W.slot_bytes(g.kind[k])].copy() if g.kind[k] else None))
    g = W.Gold(seqs)
    assert g.n == 170 == len(alone)
    idx, arena, _ = _sim.index_extract(np.frombuffer(annexb(g.nals * W.TILES), dtype=np.uint8))
    parsed, structs = _sim.parse_headers(arena, idx, fix=1)
    assert len(parsed) == W.TILES * g.n
    for j in range(W.TILES * g.n):
        seed, k, rc, kind, slot = alone[j % g.n]
        if (seed, k) in W.LEFT_OUT:
            continue
        assert int(parsed["rc"][j]) == rc, (j, seed, k)
        if kind:
            off = int(parsed["struct_off"][j])
            assert np.array_equal(structs[off:off + len(slot)], slot), (j, seed, k, kind)


def test_slice_that_reads_its_own_row(orc):
    """tests/golden/write_rows.json.gz: an IDR set to P type under lists_modification_present_flag counts the used pictures of
    a row that nothing has written; single-stepped with a cleared row it comes out as the reference wrote it"""
    from tests import _writegold as W
    fx = W.rows_fixture()
    idx, arena, _ = _sim.index_extract(np.frombuffer(annexb([bytes.fromhex(x) for x in fx["nals"]]), dtype=np.uint8))
    parsed, structs = _sim.parse_headers(arena, idx, fix=1)
    kinds = ["vps", "sps", "pps", "sh", "sh"]
    part = lambda j: structs[int(parsed["struct_off"][j]):int(parsed["struct_off"][j]) + slot_bytes(kinds[j])].copy()      # noqa: E731
    k = fx["reader"]
    slot = part(k)
    for name, value in fx["edits"]:
        slot.view(np.int32)[field_index("sh", name)] = value
    res, rbsp = _sim.write_nal(int(parsed["nal_unit_type"][k]), int(parsed["nal_layer_id"][k]), int(parsed["nal_temporal_id_plus1"][k]),
                               slot, part(1), part(2), fx["size"] * 3 // 4)
    rc, _, out = orc.rbsp_to_nal(bytes(rbsp))
    assert int(res["rc"]) == 0 and rc == fx["write_rc"] and out.hex() == fx["out"]
    assert int(res["slice_data_size"]) == fx["slice_data_size"]
