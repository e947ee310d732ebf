"""hbs_ts_mux on the CPU side: the symbols and the record size, hbs_ts_mux_psi_host and hbs_ts_mux_au_packets_host against the
plain restatement of the rule (tests/_tsmux_ref.py), and that restatement against the demultiplexer's (tests/_ts_ref.py)."""
import numpy as np
import pytest

from tests import _ts_ref as D
from tests import _tsmux_ref as R
from tests._tsmux_ref import random_case


def test_symbols_declared_and_exported():
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import EXPORTS
    from tests.test_abi_exports import declared_functions
    for name in ("hbs_ts_mux", "hbs_ts_mux_psi_host", "hbs_ts_mux_au_packets_host"):
        assert name in declared_functions()
        assert name in EXPORTS
        assert hasattr(hbs.load_library(), name)
    assert hasattr(hbs.Context, "ts_mux") and hasattr(hbs.Context, "ts_mux_async")
    assert hbs.TS_MUX_PARAMS.itemsize == 48 and hbs.TS_MUX_PARAMS == R.PARAMS and hbs.ACCESS_UNIT == R.ACCESS_UNIT
    assert (hbs.TSMUX_PCR, hbs.TSMUX_PSI_AT_IRAP, hbs.TSMUX_NO_PSI) == (R.PCR, R.PSI_AT_IRAP, R.NO_PSI) == (1, 2, 4)
    assert callable(hbs.ts_mux_psi) and callable(hbs.ts_mux_au_packets)


def random_params(rng):
    pid, pmt_pid = (int(x) for x in rng.choice(np.arange(16, 8191), size=2, replace=False))
    return R.params(pid=pid, pmt_pid=pmt_pid, packet_bytes=int(rng.choice(R.SIZES)), program_number=int(rng.integers(1, 65536)),
                    transport_stream_id=int(rng.integers(0, 65536)), flags=int(rng.integers(0, 8)), cc_es=int(rng.integers(0, 16)),
                    cc_pat=int(rng.integers(0, 16)), cc_pmt=int(rng.integers(0, 16)), pcr_lead=int(rng.integers(0, 1 << 40)))


def test_crc_of_a_known_section():
    # the check value of CRC-32/MPEG-2
    assert R.crc32(b"123456789") == 0x0376E6E7


def test_psi_host_against_the_reference():
    import hevcbitstream_amd as hbs
    rng = np.random.default_rng(31)
    edge = [R.params(pid=16, pmt_pid=8190, program_number=1, transport_stream_id=0), R.params(pid=8190, pmt_pid=16, program_number=65535,
                                                                                             transport_stream_id=65535, cc_pat=15, cc_pmt=15)]
    for prm in edge + [random_params(rng) for _ in range(300)]:
        pat, pmt = hbs.ts_mux_psi(R.params_record(prm))
        want = R.psi(prm)
        assert (pat, pmt) == want, prm
        for B in R.SIZES:
            head = b"".join(R.frame(p, B) for p in (pat, pmt))
            assert hbs.ts_find_pid(head, B, 0x24) == (prm["pid"], prm["program_number"])
        for pkt in (pat, pmt):
            n = 3 + ((pkt[6] & 0x0F) << 8 | pkt[7])
            assert R.crc32(pkt[5:5 + n]) == 0 and set(pkt[5 + n:]) == {0xFF}
    assert hbs.ts_mux_psi(pid=0x100, pmt_pid=0x1000) == R.psi(R.params())


def test_au_packets_host_against_the_reference():
    import hevcbitstream_amd as hbs
    for E in range(0, 601):
        for tf, f in ((0, 0), (1, 2), (2, 3)):
            for pcr in (False, True):
                want = R.au_packets(E, f, pcr and f != 0)
                assert hbs.ts_mux_au_packets(E, tf, pcr) == want, (E, tf, pcr)
    assert hbs.ts_mux_au_packets(1 << 40, 2, True) == R.au_packets(1 << 40, 3, True)
    assert hbs.ts_mux_au_packets(10, 3) == 0 and hbs.ts_mux_au_packets(10, -1) == 0


@pytest.mark.parametrize("B", R.SIZES)
def test_the_reference_mux_through_the_reference_demux(B):
    """the two plain loops agree with each other: AU bytes, times and random-access flags in, the same out"""
    rng = np.random.default_rng(B)
    for flags in (0, R.PCR, R.PCR | R.PSI_AT_IRAP, R.NO_PSI):
        prm = R.params(packet_bytes=B, flags=flags, cc_es=int(rng.integers(0, 16)), cc_pat=3, cc_pmt=14, pcr_lead=int(rng.integers(0, 90000)))
        stream, au, pts, dts = random_case(rng, 60, prm)
        out, au_packet, s = R.mux(stream, au, pts, dts, prm)
        assert s["error"] == 0 and len(out) == s["stream_bytes"] == s["nal_count"] * B
        es, pes, ds = D.demux(out, B, prm["pid"])
        want = b"".join(stream[int(b):int(e)].tobytes() for b, e in zip(au["unit_begin"], au["unit_end"]))
        assert es.tobytes() == want and ds["error"] == 0 and ds["reserved"] == [0, 0, 0]
        assert ds["nal_count"] == 60 and ds["nal_found"] == s["reserved"][1]
        assert pes["packet"].tolist() == au_packet[:-1].tolist()
        assert pes["out_off"].tolist() == np.concatenate([[0], np.cumsum(au["unit_end"] - au["unit_begin"])[:-1]]).tolist()
        assert pes["pts"].tolist() == pts.tolist()
        assert pes["dts"].tolist() == np.where(dts == R.NO_TIME, pts, dts).tolist()
        for k in range(60):
            f = R.time_fields(int(pts[k]), int(dts[k]))
            want_flags = D.F_ALIGN | (D.F_PTS if f else 0) | (D.F_DTS if f == 3 else 0) | (D.F_RAI if au["flags"][k] & R.AU_IRAP else 0)
            assert int(pes["flags"][k]) == want_flags, (k, f)
        if not flags & R.NO_PSI:
            import hevcbitstream_amd as hbs
            assert hbs.ts_find_pid(out[: 2 * B].tobytes(), B) == (prm["pid"], prm["program_number"])
            # every PAT and PMT: in step on their own PIDs
            for pid, cc0 in ((0, 3), (prm["pmt_pid"], 14)):
                rows = out.reshape(-1, B)[:, D.lead(B):]
                mine = rows[((rows[:, 1].astype(int) & 0x1F) << 8 | rows[:, 2]) == pid]
                assert len(mine) == s["reserved"][2] and ((mine[:, 3] & 15) == (cc0 + np.arange(len(mine))) & 15).all()


def test_the_vectorised_reference_equals_the_loop():
    rng = np.random.default_rng(77)
    for B, flags in ((188, 0), (192, R.NO_PSI), (204, R.PCR)):
        prm = R.params(packet_bytes=B, flags=flags, cc_es=9)
        stream, au, _, _ = random_case(rng, 700, prm, max_es=9)
        a, b = R.mux(stream, au, None, None, prm), R.mux_one_packet_aus(stream, au, prm)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_psi_host_refuses_bad_params():
    import hevcbitstream_amd as hbs
    lib = hbs.load_library()
    pat, pmt = np.zeros(188, dtype=np.uint8), np.zeros(188, dtype=np.uint8)

    def rc(**kw):
        p = R.params_record(R.params(**kw))
        return lib.hbs_ts_mux_psi_host(p.ctypes.data, pat.ctypes.data, pmt.ctypes.data)
    assert rc() == 0 and rc(pid=16, pmt_pid=8190) == 0
    for bad in (dict(pid=15), dict(pid=8191), dict(pid=-1), dict(pmt_pid=15), dict(pmt_pid=8191), dict(pid=0x200, pmt_pid=0x200),
                dict(packet_bytes=190), dict(packet_bytes=0), dict(reserved=1), dict(program_number=0), dict(program_number=65536),
                dict(transport_stream_id=-1), dict(transport_stream_id=65536), dict(flags=8), dict(cc_es=16), dict(cc_pat=16), dict(cc_pmt=16)):
        assert rc(**bad) == R.E_ARG, bad
    good = R.params_record(R.params())
    assert lib.hbs_ts_mux_psi_host(None, pat.ctypes.data, pmt.ctypes.data) == R.E_ARG
    assert lib.hbs_ts_mux_psi_host(good.ctypes.data, None, pmt.ctypes.data) == R.E_ARG
    assert lib.hbs_ts_mux_psi_host(good.ctypes.data, pat.ctypes.data, None) == R.E_ARG
    with pytest.raises(hbs.HbsError):
        hbs.ts_mux_psi(pid=0x100, pmt_pid=0x100)
