"""hbs_rtp_order on the CPU side: the symbols and the record layout, a fixed vector written out by hand that the plain loop of
tests/_rtp_order_ref.py must give, the loop against its vectorised restatement on random small tables, and the loop in front of
the plain loop of hbs_rtp_unpack (tests/_rtp_unpack_ref.py): a shuffled, duplicated, lossy table comes out as the in-order one."""
import numpy as np
import pytest

from tests import _rtp_order_ref as O
from tests import _rtp_unpack_ref as U


def test_symbols_declared_and_exported():
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import EXPORTS
    from tests.test_abi_exports import declared_functions
    assert "hbs_rtp_order" in declared_functions()
    assert "hbs_rtp_order" in EXPORTS
    assert hasattr(hbs.load_library(), "hbs_rtp_order")
    assert hasattr(hbs.Context, "rtp_order") and hasattr(hbs.Context, "rtp_order_async")
    assert hbs.RTP_ORDER_PARAMS.itemsize == 32 and hbs.RTP_ORDER_PARAMS == O.PARAMS
    offsets = {name: hbs.RTP_ORDER_PARAMS.fields[name][1] for name in hbs.RTP_ORDER_PARAMS.names}
    assert offsets == dict(payload_type=0, flags=4, ssrc=8, reserved=12, max_span=16, after_ext=24)
    assert (hbs.RTPO_MATCH_SSRC, hbs.RTPO_AFTER) == (O.MATCH_SSRC, O.AFTER) == (1, 2)
    prm = O.params(flags=3, max_span=77, after_ext=(1 << 48) + 5)
    assert np.array_equal(hbs.rtp_order_params(**{k: v for k, v in prm.items() if k != "reserved"}), O.params_record(prm))


FIXED_SEQS = (65534, 0, 65535, 0, 1, 3)


def fixed_table():
    packets = O.seq_packets(FIXED_SEQS) + [U.packet(b"\x40\x01\xAA", 2, 5, pt=97)]
    return U.lay_out(packets)


def test_the_fixed_vector():
    """so that the reference is not its own judge"""
    data, off, size = fixed_table()
    got = O.order(data, off, size, O.params())
    assert got["src"].tolist() == [0, 2, 1, 4, 5]
    assert got["ext"].tolist() == [(1 << 48) + x for x in (65534, 65535, 65536, 65537, 65539)]
    assert got["off"].tolist() == [int(off[i]) for i in (0, 2, 1, 4, 5)] and got["size"].tolist() == [14] * 5
    assert got["summary"] == dict(nal_count=5, nal_found=6, rbsp_bytes=(1 << 48) + 65539, stream_bytes=6, stop_reason=0, error=0,
                                  reserved=[0, 1, 1 << 32 | 1])
    # max_span one short, then out_cap one short
    short = O.order(data, off, size, O.params(max_span=5))
    assert short["summary"] == dict(nal_count=0, nal_found=6, rbsp_bytes=0, stream_bytes=6, stop_reason=0, error=O.E_CAPACITY, reserved=[0, 0, 0])
    assert O.order(data, off, size, O.params(max_span=6))["summary"]["error"] == 0
    short = O.order(data, off, size, O.params(), out_cap=4)
    assert short["summary"] == dict(got["summary"], error=O.E_CAPACITY) and len(short["off"]) == 0


def test_the_fixed_vector_after():
    """the sequence continues behind 2^48 + 3 * 65536 + 65534: the first packet is that one again, and late"""
    data, off, size = fixed_table()
    after = (1 << 48) + 3 * 65536 + 65534
    got = O.order(data, off, size, O.params(flags=O.AFTER, after_ext=after))
    assert got["src"].tolist() == [2, 1, 4, 5]
    assert got["ext"].tolist() == [after + 1, after + 2, after + 3, after + 5]
    # base = after_ext + 1: span 5 of which 4 are kept; one late = 6 - 4 - 1 duplicate
    assert got["summary"] == dict(nal_count=4, nal_found=6, rbsp_bytes=after + 5, stream_bytes=5, stop_reason=0, error=0,
                                  reserved=[0, 1, 1 << 32 | 1])
    # a leading loss counts: behind after - 2 the packets 65533 (lost) .. 3
    got = O.order(data, off, size, O.params(flags=O.AFTER, after_ext=after - 2))
    assert got["src"].tolist() == [0, 2, 1, 4, 5] and got["ext"][0] == after
    assert got["summary"]["stream_bytes"] == 7 and got["summary"]["reserved"] == [0, 2, 1 << 32 | 1]


def test_a_fault_reports_the_lowest_entry():
    data, off, size = fixed_table()
    size2 = size.copy()
    size2[3], size2[5] = 11, 11
    got = O.order(data, off, size2, O.params())
    assert got["summary"] == dict(O.empty_summary(), error=O.E_ARG, reserved=[4, 0, 0]) and len(got["off"]) == 0


def random_seq_table(rng):
    """a small table of packets whose seqs are a shuffled walk or plain random 16-bit values (ext may fall below 2^48), some of
    another payload type or ssrc, with the difference 0x8000 among the steps"""
    n = int(rng.integers(0, 40))
    kind = int(rng.integers(0, 4))
    if kind == 0:
        seqs = rng.integers(0, 65536, size=n)
    elif kind == 1:
        seqs = int(rng.integers(0, 65536)) - np.arange(n) * int(rng.integers(1, 300))
    else:
        start = int(rng.integers(0, 65536))
        walk = start + O.arrival_order(n, int(rng.integers(0, 9)), rng)
        seqs = np.concatenate([walk, walk[: n // 4]])[rng.permutation(n + n // 4)[:n]] if kind == 3 and n else walk
    seqs = np.asarray(seqs, dtype=np.int64) & 0xFFFF
    if n > 2 and rng.random() < 0.3:
        k = int(rng.integers(1, n))
        seqs[k] = (seqs[k - 1] + 0x8000) & 0xFFFF
    other = rng.random(n) < 0.2
    match = rng.random() < 0.5
    packets = []
    for k in range(n):
        pt, ssrc = 96, O.SSRC
        if other[k]:
            pt, ssrc = (96, 0x77) if match and k % 2 else (97, O.SSRC)
        packets += O.seq_packets([seqs[k]], pt=pt, ssrc=ssrc)
    prm = O.params(flags=O.MATCH_SSRC if match else 0, max_span=int(rng.integers(1, 70000)) if rng.random() < 0.3 else 1 << 33)
    if rng.random() < 0.5:
        near = (1 << 48) + int(rng.integers(0, 1 << 20)) if rng.random() < 0.8 else int(rng.integers(1 << 48, (1 << 62) + 1))
        if n and rng.random() < 0.7:
            near = (near & ~0xFFFF) | ((int(seqs[0]) - int(rng.integers(-5, 6))) & 0xFFFF)
            near = max(near, 1 << 48)
        prm.update(flags=prm["flags"] | O.AFTER, after_ext=near)
    return packets, seqs, ~other, prm


def test_the_loop_against_the_vectorised_restatement():
    rng = np.random.default_rng(1701)
    seen = dict(below=0, half=0, capacity=0, late=0, moved=0, duplicates=0)
    for _ in range(3000):
        packets, seqs, accepted, prm = random_seq_table(rng)
        data, off, size = U.lay_out(packets)
        a = O.order(data, off, size, prm)
        b = O.order_plain(seqs, accepted, prm, off, size)
        assert a["summary"] == b["summary"], (seqs, prm, a["summary"], b["summary"])
        if a["summary"]["error"] == 0:
            for k in ("off", "size", "src", "ext"):
                assert np.array_equal(a[k], b[k]), (k, seqs, prm)
            assert len(a["ext"]) < 2 or (np.diff(a["ext"].astype(np.int64)) > 0).all()
        s = a["summary"]
        seen["capacity"] += s["error"] == O.E_CAPACITY
        seen["below"] += len(a["ext"]) > 0 and int(a["ext"][0]) < 1 << 48
        seen["half"] += len(seqs) > 1 and bool((((seqs[1:] - seqs[:-1]) & 0xFFFF) == 0x8000).any())
        seen["late"] += s["error"] == 0 and s["nal_found"] - s["nal_count"] - (s["reserved"][2] >> 32) > 0
        seen["moved"] += s["reserved"][2] & 0xFFFFFFFF > 0
        seen["duplicates"] += s["reserved"][2] >> 32 > 0
    assert all(v > 20 for v in seen.values()), seen


def in_order_packets(rng, n, **kw):
    packets, nals, _, _ = U.random_packets(rng, n, **kw)
    return packets, nals


@pytest.mark.parametrize("seed,seq", ((1, None), (2, 65500), (3, 65535 - 150)))
def test_order_then_unpack_is_the_unpack_of_the_in_order_table(seed, seq):
    rng = np.random.default_rng(seed)
    packets, nals = in_order_packets(rng, 300, seq=seq)
    want = U.unpack(*U.lay_out(packets), U.params())
    assert want["nals"] == nals and want["summary"]["reserved"][2] == 0
    arrived, origin = O.arrive(packets, rng, window=8, duplicates=12, others=0.05)
    data, off, size = U.lay_out(arrived, rng)
    assert U.unpack(data, off, size, U.params())["nals"] != nals              # the arrival order does not unpack
    got = O.order(data, off, size, O.params())
    assert [origin[i] for i in got["src"]] == list(range(len(packets)))
    s = got["summary"]
    assert s["nal_count"] == len(packets) == s["stream_bytes"] and s["reserved"][1] == 0 and s["reserved"][2] >> 32 == 12 and s["reserved"][2] & 0xFFFFFFFF > 0
    back = U.unpack(data, got["off"], got["size"], U.params())
    assert back["nals"] == nals and np.array_equal(back["out"], want["out"]) and back["summary"] == want["summary"]
    assert np.array_equal(back["nal_au"], want["nal_au"]) and np.array_equal(back["au_ts"], want["au_ts"])


def test_with_a_loss_set_it_is_the_unpack_of_the_in_order_table_without_those_entries():
    rng = np.random.default_rng(4)
    packets, _ = in_order_packets(rng, 300, seq=65400)
    lose = sorted(int(x) for x in rng.choice(np.arange(1, 299), size=15, replace=False))
    left = [p for i, p in enumerate(packets) if i not in lose]
    want = U.unpack(*U.lay_out(left), U.params())
    arrived, origin = O.arrive(packets, rng, window=8, duplicates=9, lose=lose, others=0.05, other_kind="ssrc")
    data, off, size = U.lay_out(arrived, rng)
    got = O.order(data, off, size, O.params(flags=O.MATCH_SSRC))
    assert [origin[i] for i in got["src"]] == [i for i in range(300) if i not in lose]
    assert got["summary"]["stream_bytes"] == 300 and got["summary"]["reserved"][1] == 15
    back = U.unpack(data, got["off"], got["size"], U.params(flags=U.MATCH_SSRC))
    assert np.array_equal(back["out"], want["out"]) and back["summary"] == want["summary"]
    assert np.array_equal(back["nal_au"], want["nal_au"]) and np.array_equal(back["au_ts"], want["au_ts"])
