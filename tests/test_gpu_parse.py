"""Parity tests for K4 (header parse, one NAL per lane) through the C ABI:
NAL header, VPS/SPS/PPS/slice-segment-header structs and slice payload location
against the oracle parser, on streams from tests/hevc_synth.py."""
import json
import os
import time

import numpy as np
import pytest

from tests import _orc
from tests._parsecmp import compare, oracle_pass
from tests.hevc_synth import Synth, annexb, stream_4k30
from tests.test_sim_parse_logic import broken, sequence

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ctx():
    import hevcbitstream_amd as hbs
    c = hbs.Context(0)
    yield c
    c.close()


def gpu_parse(ctx, stream_bytes):
    import torch
    s = np.frombuffer(stream_bytes, dtype=np.uint8).copy()
    d = torch.from_numpy(s).cuda()
    index, rbsp, summary, cap = ctx.alloc_outputs(d.numel())
    ctx.index_extract_async(d, index, cap, rbsp, summary)
    sm = ctx.read_summary(summary)
    n = int(sm["nal_count"])
    parsed, structs = ctx.parse_headers(rbsp, index, n, poison=0xA5)      # the parse has to clear every struct it fills
    import hevcbitstream_amd as hbs
    idx = index[: n * 32].cpu().numpy().view(hbs.NAL_ENTRY)
    return s, idx, rbsp[: int(sm["rbsp_bytes"])].cpu().numpy(), parsed, structs.cpu().numpy()


def run(ctx, nals):
    s, idx, arena, parsed, structs = gpu_parse(ctx, annexb(nals))
    assert len(idx) == len(nals)
    compare(parsed, structs, arena, idx, oracle_pass(nals))


def test_rich_sequences(ctx):
    # many sequences in ONE stream would share parser state; the reference parses one stream at a time too
    for seed in range(40):
        run(ctx, sequence(seed))


def test_long_mixed_stream(ctx):
    """one stream with 60 parameter-set changes and ~700 slices: context resolution across the stream"""
    nals = []
    for seed in range(200, 260):
        nals += sequence(seed)
    run(ctx, nals)


def test_broken_slices_and_parameter_sets(ctx):
    for seed in range(25):
        run(ctx, broken(sequence(seed), np.random.RandomState(1000 + seed), lambda t: t not in (33, 34)))
    for seed in range(25):
        g = Synth(seed, rich=True)
        rng = np.random.RandomState(2000 + seed)
        seq = [g.vps(), g.sps_nal(int(rng.randint(64, 4096)), int(rng.randint(64, 2304))), g.pps_nal(), g.vps()]
        run(ctx, broken(seq, rng, lambda t: True))


def test_sequential_batch_is_the_reference_on_forbidden_streams():
    """hbs_ctx_set_sequential_parse: a batch walked NAL after NAL with one set of RPS tables matches the oracle (= the
    reference) even where slices name a set their cut-short SPS does not have -- the five streams on which the default,
    independent parse reads zeros instead -- and on ordinary ones"""
    import hevcbitstream_amd as hbs
    c = hbs.Context(0)
    c.set_sequential_parse(True)
    try:
        for seed in (1036, 1064, 1320, 1496, 5224, 3, 4):
            nals = broken(sequence(seed), np.random.RandomState(7 * seed + 2), lambda t: True) if seed > 100 else sequence(seed)
            run(c, nals)
        nals = []                                            # a longer stream: parameter sets changing under way
        for seed in range(300, 312):
            nals += sequence(seed)
        run(c, nals)
    finally:
        c.close()


def test_default_batch_is_the_reference_on_forbidden_streams():
    """the DEFAULT batch parse on the same streams: a slice that names a set its SPS does not have (or rewrites one of its
    rows) raises a flag on the device and the batch is walked again in order behind the parallel parse -- no switch to set,
    and ordinary streams do not pay for it (the gated kernel returns at once)"""
    import hevcbitstream_amd as hbs
    c = hbs.Context(0)
    try:
        for seed in (1036, 1064, 1320, 1496, 5224, 3, 4):
            nals = broken(sequence(seed), np.random.RandomState(7 * seed + 2), lambda t: True) if seed > 100 else sequence(seed)
            run(c, nals)
        nals = []                                            # several sequences in one batch, the forbidden ones among them
        for seed in (300, 1036, 301, 1320, 302, 5224, 303):
            nals += broken(sequence(seed), np.random.RandomState(7 * seed + 2), lambda t: True) if seed > 1000 else sequence(seed)
        run(c, nals)
        for seed in range(6000, 6120):                       # parameter sets corrupted too: the family the divergence was found in
            run(c, broken(sequence(seed), np.random.RandomState(7 * seed + 2), lambda t: True))
    finally:
        c.close()


def test_ten_nal_fixture(ctx):
    data = open(os.path.join(HERE, "golden", "ten_nal.hevc"), "rb").read()
    idx = json.load(open(os.path.join(HERE, "golden", "ten_nal.index.json")))
    run(ctx, [data[s:e] for s, e, _ in idx[:4]])


def test_golden_struct_dumps(ctx):
    """reference answers (parse_vectors.json) straight against the GPU parse"""
    gold = json.load(open(os.path.join(HERE, "golden", "parse_vectors.json")))
    from tests import _orc
    for seq in gold[:12]:
        nals = [bytes.fromhex(st["nal"]) for st in seq["steps"]]
        s, idx, arena, parsed, structs = gpu_parse(ctx, annexb(nals))
        for k, st in enumerate(seq["steps"]):
            assert int(parsed["rc"][k]) == st["rc"]
            t = (nals[k][0] >> 1) & 0x3F
            kind = "sh" if (t <= 9 or 16 <= t <= 21) else {32: "vps", 33: "sps", 34: "pps"}.get(t)
            if kind is None:
                continue
            size = _orc.layout()[_orc.STRUCT_TYPES[kind]]["size"]
            got = structs[int(parsed["struct_off"][k]): int(parsed["struct_off"][k]) + size].view(np.int32)
            want = np.zeros(size // 4, dtype=np.int32)
            for i, v in st["structs"][kind]:
                want[i] = v
            assert np.array_equal(got, want), (seq["seed"], k, kind)


def test_config3_4k30_100k_nals(ctx):
    """Config 3: synthetic 3840x2160 stream, ~100k NALs (12.5k pictures x 8 slice segments + parameter
    sets every 60 pictures).  Full field parity of ALL 100 627 NALs -- rc, NAL header, every struct member, slice payload --
    against the oracle's read_hevc_nal_unit fed the NALs in stream order (a few seconds), and against the compiled reference
    itself when its prebuilt library travelled with the tree."""
    t0 = time.time()
    stream, n = stream_4k30(11, n_pictures=12500, slices_per_picture=8, idr_every=60, payload_bytes=(60, 120))
    s, idx, arena, parsed, structs = gpu_parse(ctx, stream)
    assert len(idx) == n and n > 100000
    assert (parsed["rc"] >= 0).all()
    nals = [bytes(s[int(a):int(b)]) for a, b in zip(idx["start"], idx["end"])]
    compare(parsed, structs, arena, idx, oracle_pass(nals))
    from tests import _orc
    if _orc.reference() is not None:
        compare(parsed, structs, arena, idx, oracle_pass(nals, parser=_orc.ReferenceHevc()))
    # whole stream: slice_data_size + header bytes + 1 == rbsp_len for every slice
    sl = (parsed["nal_unit_type"] == 1) | (parsed["nal_unit_type"] == 19)
    assert (parsed["slice_data_size"][sl] + parsed["slice_data_off"][sl].astype(np.int64) == idx["rbsp_len"][sl]).all()


def test_out_of_spec_slices_are_walked_again_by_themselves(ctx):
    """A 4K30-style batch of ~16 k NALs in which one slice in a hundred is an IDR coded as a P slice: its header reads the RPS
    row the last slice with an own set left behind (hevc_stream.c:35-59 on the file-static tables), which the parallel parse
    does not know.  Only those slices are walked again, each with the true row handed in (hbs_parse_fix.h); every NAL of
    the batch must equal the oracle's sequential parse -- and the batch parse alone must NOT (the test has teeth)."""
    stream, n = stream_4k30(21, n_pictures=2000, slices_per_picture=8, idr_every=60, payload_bytes=(60, 120), forbidden_every=100)
    s, idx, arena, parsed, structs = gpu_parse(ctx, stream)
    assert len(idx) == n
    nals = [bytes(s[int(a):int(b)]) for a, b in zip(idx["start"], idx["end"])]
    exp = oracle_pass(nals)
    compare(parsed, structs, arena, idx, exp)
    from tests import _sim
    p0, s0 = _sim.parse_headers(arena, idx, fix=0)                      # the batch parse alone, single-stepped on the CPU
    with pytest.raises(AssertionError):
        compare(p0, s0, arena, idx, exp)


def test_write_headers_batch_roundtrip(ctx):
    """K5 over a whole parsed batch (config-3 style stream, ~8k NALs): VPS and PPS come back bit for bit
    (SURVEY: "round-trips VPS/PPS exactly"), an SPS comes back without its trailing bits and unfinished
    last byte: a prefix of the RBSP it was parsed from.  Slices: the reference's writer re-codes some fields; when the
    compiled reference travelled with the tree, every slice is held against what it writes from the same NAL (bytes,
    rbsp_size, slice_data_size); the golden batches of tests/test_gpu_write.py hold them against recorded answers."""
    stream, n = stream_4k30(17, n_pictures=1000, slices_per_picture=8, idr_every=60, payload_bytes=(60, 120))
    s, idx, arena, parsed, structs = gpu_parse(ctx, stream)
    assert (parsed["rc"] >= 0).all()
    import torch
    cap = 256
    written, out = ctx.write_headers(parsed, torch.from_numpy(structs).cuda(), len(parsed), cap)
    out = out.cpu().numpy()
    assert (written["rc"] == 0).all()
    kinds = {32: 0, 33: 0, 34: 0, "slice": 0}
    ref = _orc.ReferenceHevc() if _orc.reference() is not None else None
    size = (4 * cap + 2) // 3                                   # the reference writes into size * 3 / 4 bytes (hevc_stream.c:1266)
    assert size * 3 // 4 == cap
    for k in range(len(parsed)):
        t = int(parsed["nal_unit_type"][k])
        got = bytes(out[k * cap:k * cap + int(written["rbsp_size"][k])])
        rb = bytes(arena[int(idx["rbsp_off"][k]):int(idx["rbsp_off"][k]) + int(idx["rbsp_len"][k])])
        if t in (32, 34):
            assert got == rb, (k, t)
            kinds[t] += 1
        elif t == 33:
            assert len(got) >= len(rb) - 2 and rb.startswith(got), (k, got.hex(), rb.hex())
            kinds[t] += 1
        else:
            assert 3 <= len(got) < cap and got[:2] == rb[:2], (k, len(got))
            kinds["slice"] += 1
        if ref is not None:                                    # (stream_4k30 holds VPS, SPS, PPS and slices, nothing else: the reference writes every one)
            nal = bytes(s[int(idx["start"][k]):int(idx["end"][k])])
            assert ref.read(nal) == int(parsed["rc"][k]), k
            if t not in (32, 33, 34):
                wrc, out_nal, sds = ref.write(size)
                assert wrc >= 0, (k, wrc)
                want = _orc.reference().nal_to_rbsp(out_nal)[3]
                assert got == want and not out[k * cap + len(got):(k + 1) * cap].any(), (k, got.hex(), want.hex())
                assert int(written["slice_data_size"][k]) == sds, (k, int(written["slice_data_size"][k]), sds)
                kinds["held to the reference"] = kinds.get("held to the reference", 0) + 1
    assert min(kinds.values()) > 0, kinds
    assert kinds.get("held to the reference", kinds["slice"]) == kinds["slice"], kinds      # all of them, or none (no compiled reference here)
