#!/usr/bin/env python3
"""Kernel time of hbs_ts_mux (the library's HIP events around all of a call's launches, hbs_ctx_kernel_ms) on the bench stream
-- S(0x1234, n) of ~10 KiB NALs, 16 GiB by default, cut into access units of --au-nals NALs -- and on a stream of access units
of ~1 KiB (scripts/nal_sweep.py's shape, one NAL an AU, 2 GiB by default): 188-byte packets, a PTS and a DTS on every AU, a
PCR, PAT + PMT in front of every 32nd AU (flagged IRAP).  Next to each, in the same process, hbs_ts_demux (with its PES table)
on the very stream the mux produced.  Traffic = the bytes read + the bytes written: for the mux the AUs' bytes and the packets,
for the demux the packets and the elementary stream; the AU table and the times (80 B an AU, read by each plan pass), the
8 B an AU of scratch and the 32 B a PES packet of table are not counted.  Fractions of the 8 TB/s peak.
    python scripts/tsmux_time.py [--gib 16] [--small-gib 2] [--reps 5] [--au-nals 8]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_PEAK_GBS = 8000.0
PID = 0x100


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=16.0)
    ap.add_argument("--small-gib", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--au-nals", type=int, default=8)
    args = ap.parse_args()
    import numpy as np
    import torch
    import hevcbitstream_amd as hbs
    from scripts.nal_sweep import make_stream

    ctx = hbs.Context(0)
    dev = torch.device("cuda", 0)
    rows = []

    def shapes():
        n = int(round(104_858 * args.gib))
        g = ctx.synth_stream(0x1234, n, 0)
        yield "S(0x1234, %d) ~10 KiB NALs, AUs of %d NALs" % (n, args.au_nals), g["stream"][: g["stream_bytes"]], n, args.au_nals
        del g
        arena, total, idx, n, stream, sb = make_stream(torch, np, ctx, 1024, int(args.small_gib * 2**30))
        del arena, idx
        yield "random payload, AUs of one ~1 KiB NAL", stream[:sb], n, 1

    def timed(call):
        ctx.enable_timing(True)
        call()                                          # warm-up
        for _ in range(args.reps):
            call()
        ms = sorted(ctx.kernel_ms_back(b) for b in range(args.reps))
        ctx.enable_timing(False)
        return ms

    for name, stream, n, per in shapes():
        sb = stream.numel()
        ent, _, s = ctx.index_extract(stream, index_cap=n + 16, want_rbsp=False)
        assert len(ent) == n, (len(ent), n)
        ends = ent["end"].astype(np.uint64)
        n_aus = (n + per - 1) // per
        au = np.zeros(n_aus, dtype=hbs.ACCESS_UNIT)
        last = np.minimum(np.arange(n_aus) * per + per, n) - 1
        au["unit_end"] = ends[last]
        au["unit_begin"][1:] = au["unit_end"][:-1]
        au["flags"] = np.where(np.arange(n_aus) % 32 == 0, hbs.AU_IRAP, 0)
        es_bytes = int(au["unit_end"][-1])
        dts = (np.arange(n_aus, dtype=np.uint64) * np.uint64(3003)) & np.uint64((1 << 33) - 1)
        pts = (dts + np.uint64(6006)) & np.uint64((1 << 33) - 1)
        del ent
        d_au, d_pts, d_dts = (torch.from_numpy(x.view(np.uint8).copy()).to(dev) for x in (au, pts, dts))
        prm = hbs.ts_mux_params(pid=PID, flags=hbs.TSMUX_PCR | hbs.TSMUX_PSI_AT_IRAP, pcr_lead=9000)
        summ = torch.zeros(64, dtype=torch.uint8, device=dev)
        assert ctx.ts_mux_async(stream, sb, d_au, n_aus, d_pts, d_dts, prm, None, None, summ) == 0
        plan = ctx.read_summary(summ)
        assert int(plan["error"]) == 0 and int(plan["rbsp_bytes"]) == es_bytes, plan
        out_bytes, packets = int(plan["stream_bytes"]), int(plan["nal_count"])
        out = torch.empty(out_bytes + 16, dtype=torch.uint8, device=dev)
        au_packet = torch.empty(n_aus + 1, dtype=torch.int32, device=dev)

        def mux():
            assert ctx.ts_mux_async(stream, sb, d_au, n_aus, d_pts, d_dts, prm, out, au_packet, summ, out_cap=out_bytes) == 0
        mux_ms = timed(mux)
        sm = ctx.read_summary(summ)
        assert int(sm["error"]) == 0 and int(sm["stream_bytes"]) == out_bytes and int(sm["nal_found"]) == n_aus, sm
        assert hbs.ts_find_pid(out[: 2 * 188].cpu().numpy(), 188) == (PID, 1)

        back = torch.empty(es_bytes + 16, dtype=torch.uint8, device=dev)
        pes = torch.empty(n_aus * 32, dtype=torch.uint8, device=dev)

        def demux():
            assert ctx.ts_demux_async(out, out_bytes, 188, PID, back, pes, summ, out_cap=es_bytes, pes_cap=n_aus) == 0
        demux_ms = timed(demux)
        sm = ctx.read_summary(summ)
        assert int(sm["error"]) == 0 and int(sm["stream_bytes"]) == es_bytes and int(sm["nal_count"]) == n_aus and int(sm["reserved"][1]) == 0, sm
        # the round trip: the AUs touch, so the elementary stream is the input up to the last AU's end
        assert torch.equal(back[:es_bytes], stream[:es_bytes])
        got = pes.cpu().numpy().view(hbs.TS_PES)
        assert np.array_equal(got["pts"], pts) and np.array_equal(got["dts"], dts) and np.array_equal(got["out_off"], au["unit_begin"])
        assert np.array_equal(got["packet"], au_packet.cpu().numpy().view(np.uint32)[:-1])

        d_med = demux_ms[len(demux_ms) // 2]
        for call, ms, inb, outb in (("hbs_ts_mux", mux_ms, es_bytes, out_bytes), ("hbs_ts_demux of its output", demux_ms, out_bytes, es_bytes)):
            med = ms[len(ms) // 2]
            traffic = inb + outb
            row = dict(stream=name, call=call, aus=n_aus, packets=packets, in_bytes=inb, out_bytes=outb, kernel_ms_min=round(ms[0], 4),
                       kernel_ms_median=round(med, 4), traffic_bytes=traffic, gbs=round(traffic / med / 1e6, 1),
                       fraction_of_8tbs=round(traffic / med / 1e6 / HBM_PEAK_GBS, 3), time_over_demux=round(med / d_med, 3))
            rows.append(row)
            print("%-44s %-28s %8.3f ms (min %8.3f)  %6.2f GiB in  %6.2f GiB out  %7.0f GB/s  %.3f of 8 TB/s (bytes read + bytes written)  %.3f x the demux's time"
                  % (name, call, med, ms[0], inb / 2**30, outb / 2**30, row["gbs"], row["fraction_of_8tbs"], row["time_over_demux"]), flush=True)
        del out, back, pes, stream, d_au, d_pts, d_dts, au_packet
        torch.cuda.empty_cache()
    print(json.dumps({"tsmux_time": rows, "source_digest": hbs.source_digest()}))


if __name__ == "__main__":
    main()
