#!/usr/bin/env python3
"""Kernel time of hbs_ts_demux (the library's HIP events around all of a call's launches, hbs_ctx_kernel_ms) on a transport
stream of 188-byte packets with 184-byte payloads and one PES start (a 14-byte header with a PTS) every 55 packets of the PID
-- 4 GiB by default, one period of 352 000 packets built vectorised in numpy and repeated on the device -- with every packet
on the PID and with nine in ten on it (the others on another PID).  Traffic = the stream read once + the output written; the
header bytes the plan passes read again and the 32 B a PES packet of table are not counted.  In the same process:
hbs_filter_annexb keep-all on ~128-byte NALs (scripts/nal_sweep.py's shape, 2 GiB by default), the nearest existing copy of
many short runs.  Fractions of the 8 TB/s peak.
    python scripts/ts_time.py [--gib 4] [--small-gib 2] [--reps 5]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_PEAK_GBS = 8000.0
PID = 0x100
PERIOD = 352_000            # packets: a multiple of 8800, in which 7920 = 144 * 55 = 495 * 16 packets are on the PID at nine in ten


def period(np, share_all):
    """PERIOD packets as an (n, 188) uint8 array; continuity counters and PES starts come out periodic"""
    rng = np.random.default_rng(7)
    a = rng.integers(0, 256, size=(PERIOD, 188), dtype=np.uint8)
    i = np.arange(PERIOD)
    on = np.ones(PERIOD, bool) if share_all else (i % 10) != 9
    k = np.cumsum(on) - 1                                   # number of the packet among the PID's
    pes = on & (k % 55 == 0)
    pid = np.where(on, PID, 0x101)
    a[:, 0] = 0x47
    a[:, 1] = (pes.astype(np.int64) << 6) | (pid >> 8)
    a[:, 2] = pid & 0xFF
    a[:, 3] = 0x10 | np.where(on, k & 15, i & 15)
    rows = np.flatnonzero(pes)
    t = (3003 * (k[rows] // 55)) & ((1 << 33) - 1)
    head = np.stack([0 * t, 0 * t, 0 * t + 1, 0 * t + 0xE0, 0 * t, 0 * t, 0 * t + 0x84, 0 * t + 0x80, 0 * t + 5,
                     0x21 | ((t >> 30) & 7) << 1, (t >> 22) & 0xFF, ((t >> 15) & 0x7F) << 1 | 1, (t >> 7) & 0xFF, (t & 0x7F) << 1 | 1], axis=1)
    a[rows, 4:18] = head
    return a, int(on.sum()) * 184 - 14 * len(rows), len(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--small-gib", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    import hevcbitstream_amd as hbs
    from scripts.nal_sweep import make_stream

    ctx = hbs.Context(0)
    dev = torch.device("cuda", 0)
    rows = []

    def timed(call):
        ctx.enable_timing(True)
        call()                                          # warm-up
        for _ in range(args.reps):
            call()
        ms = sorted(ctx.kernel_ms_back(b) for b in range(args.reps))
        ctx.enable_timing(False)
        return ms

    results = []
    reps_of_period = max(1, int(args.gib * 2**30) // (PERIOD * 188))
    for name, share_all in (("every packet on the PID", True), ("nine packets in ten on the PID", False)):
        a, es_bytes, n_pes = period(np, share_all)
        ts = torch.from_numpy(a.reshape(-1)).to(dev).repeat(reps_of_period)
        nbytes, out_bytes, pes_count = ts.numel(), es_bytes * reps_of_period, n_pes * reps_of_period
        out = torch.empty(out_bytes + 16, dtype=torch.uint8, device=dev)
        pes = torch.empty(pes_count * 32, dtype=torch.uint8, device=dev)
        summ = torch.zeros(64, dtype=torch.uint8, device=dev)

        def demux():
            assert ctx.ts_demux_async(ts, nbytes, 188, PID, out, pes, summ, out_cap=out_bytes, pes_cap=pes_count) == 0
        ms = timed(demux)
        sm = ctx.read_summary(summ)
        assert int(sm["error"]) == 0 and int(sm["stream_bytes"]) == out_bytes and int(sm["nal_count"]) == pes_count, sm
        assert int(sm["reserved"][1]) == 0 and int(sm["reserved"][2]) == 0, sm
        # the first period against numpy
        keep = a[(a[:, 1].astype(np.int64) & 0x1F) << 8 | a[:, 2] == PID]
        want = np.concatenate([r[18:] if r[1] & 0x40 else r[4:] for r in keep[:2000]])
        assert np.array_equal(out[: len(want)].cpu().numpy(), want)
        results.append(("hbs_ts_demux, " + name, ms, nbytes + out_bytes, nbytes, out_bytes))
        del ts, out, pes
        torch.cuda.empty_cache()

    arena, total, idx, n, stream, sb = make_stream(torch, np, ctx, 128, int(args.small_gib * 2**30))
    del arena, idx
    stream = stream[:sb]
    ent, _, s = ctx.index_extract(stream, index_cap=n + 16, want_rbsp=False)
    assert len(ent) == n
    d_idx = torch.from_numpy(ent.view(np.uint8).copy()).to(dev)
    unit_bytes = int(ent["end"][-1])
    back = torch.empty(sb + 16, dtype=torch.uint8, device=dev)
    io = torch.empty(n * 32, dtype=torch.uint8, device=dev)
    summ = torch.zeros(64, dtype=torch.uint8, device=dev)
    rule = ctx.nal_filter()

    def flt():
        ctx.filter_annexb_async(stream, sb, d_idx, n, back, io, summ, rule=rule, out_cap=sb)
    ms = timed(flt)
    sm = ctx.read_summary(summ)
    assert int(sm["error"]) == 0 and int(sm["stream_bytes"]) == unit_bytes, sm
    results.append(("hbs_filter_annexb keep-all, ~128-byte NALs", ms, 2 * unit_bytes, sb, unit_bytes))

    for call, ms, traffic, inb, outb in results:
        med = ms[len(ms) // 2]
        row = dict(call=call, in_bytes=inb, out_bytes=outb, kernel_ms_min=round(ms[0], 4), kernel_ms_median=round(med, 4),
                   traffic_bytes=traffic, gbs=round(traffic / med / 1e6, 1), fraction_of_8tbs=round(traffic / med / 1e6 / HBM_PEAK_GBS, 3))
        rows.append(row)
        print("%-48s %8.3f ms (min %8.3f)  %6.2f GiB in  %6.2f GiB out  %7.0f GB/s  %.3f of 8 TB/s (bytes read + bytes written)"
              % (call, med, ms[0], inb / 2**30, outb / 2**30, row["gbs"], row["fraction_of_8tbs"]), flush=True)
    print(json.dumps({"ts_time": rows, "source_digest": hbs.source_digest()}))


if __name__ == "__main__":
    main()
