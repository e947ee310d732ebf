#!/usr/bin/env python3
"""Kernel time of hbs_au_times (the library's HIP events around all of a call's launches, hbs_ctx_kernel_ms; median of --reps
calls after a warm-up, one process), next to hbs_access_units on the same batch in the same process:
  (a) the AU table of BASELINE config 3's 4K30 stream (12 500 AUs),
  (b) the AU tables of fabricated records with a picture every 8 NALs (scripts/au_time.py's),
each with the picture order counts of GOP-8 and of GOP-32 B-pyramids written into it (the streams themselves code no reordered
pictures), with all four outputs and as a plan.  There is nothing else to measure the call against: the figure is the ratio to
hbs_access_units.  Algorithmic bytes: 64 B an AU read (two words of each record: whole lines), 24 B an AU written; the call as
built also writes 17 B an AU of scratch and reads 29 B of it.
    python scripts/autimes_time.py [--reps 21] [--nals 16777216,134217728] [--pictures 12500]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_PEAK_GBS = 8000.0


def pyramid_offsets(gop):
    """decode order inside a GOP: the anchor, then the middles, depth first (1-based offsets from the GOP in front)"""
    def mid(lo, hi):
        m = (lo + hi) // 2
        return [] if m == lo else [m] + mid(lo, m) + mid(m, hi)
    return [gop] + mid(0, gop)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--nals", default="16777216,134217728")
    ap.add_argument("--pictures", type=int, default=12500)
    args = ap.parse_args()
    import numpy as np
    import torch
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import COMPACT, PARSED, SUMMARY, ACCESS_UNIT
    from hevcbitstream_amd.hevc_synth import stream_4k30

    ctx = hbs.Context(0)
    dev = torch.device("cuda", 0)
    rows = []

    def timed(call):
        ctx.enable_timing(True)
        call()
        for _ in range(args.reps):
            call()
        ms = sorted(ctx.kernel_ms_back(b) for b in range(args.reps))
        ctx.enable_timing(False)
        return ms[len(ms) // 2], ms[0]

    def access_units(index, parsed, compact, structs, n):
        """-> (median ms, min ms, the AU table on the device, AUs)"""
        summ = torch.zeros(SUMMARY.itemsize, dtype=torch.uint8, device=dev)
        assert ctx.access_units_async(index, parsed, compact, structs, n, None, 0, None, None, summ) == 0
        aus = int(ctx.read_summary(summ)["nal_count"])
        au = torch.empty(max(aus, 1) * ACCESS_UNIT.itemsize, dtype=torch.uint8, device=dev)
        nal_au = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        carry = torch.zeros(16, dtype=torch.uint8, device=dev)
        med, lo = timed(lambda: ctx.access_units_async(index, parsed, compact, structs, n, au, aus, nal_au, carry, summ))
        assert int(ctx.read_summary(summ)["error"]) == 0
        return med, lo, au, aus

    def au_times(batch, au, aus, a_med):
        words = au.view(torch.int32).reshape(-1, 16)                # word 11: pic_order_cnt
        a = torch.arange(aus, device=dev, dtype=torch.int64)
        dts, pts = (torch.empty(aus, dtype=torch.int64, device=dev) for _ in range(2))
        order, display = (torch.empty(aus, dtype=torch.int32, device=dev) for _ in range(2))
        summ = torch.zeros(SUMMARY.itemsize, dtype=torch.uint8, device=dev)
        prm = hbs.au_times_params(tick=3003, base_time=90000)
        for gop in (8, 32):
            perm = torch.tensor(pyramid_offsets(gop), device=dev, dtype=torch.int64)
            poc = torch.where(a == 0, torch.zeros_like(a), ((a - 1) // gop) * gop + perm[(a - 1) % gop])
            words[:aus, 11] = poc.to(torch.int32)
            med, lo = timed(lambda: ctx.au_times_async(au, aus, prm, summ, dts, pts, order, display))
            s = ctx.read_summary(summ)
            assert int(s["error"]) == 0 and int(s["nal_count"]) == aus and 0 < int(s["reserved"][1]) <= gop, s
            assert bool((pts >= dts).all()) and bool((order.to(torch.int64).sort().values == a).all())
            if int(s["nal_found"]) == 1:                                # one segment: the slot is the rank of the POC
                assert bool((order.to(torch.int64) == poc.argsort().argsort()).all()) and int(s["reserved"][1]) == gop.bit_length() - 1
            p_med, p_lo = timed(lambda: ctx.au_times_async(au, aus, prm, summ))
            algo, moved = (64 + 24) * aus, (64 + 24 + 17 + 29 + 4) * aus
            rows.append(dict(batch=batch, aus=aus, gop=gop, segments=int(s["nal_found"]), au_times_ms_median=round(med, 4), au_times_ms_min=round(lo, 4),
                             plan_ms_median=round(p_med, 4), plan_ms_min=round(p_lo, 4), access_units_ms_median=round(a_med, 4),
                             ratio_to_access_units=round(med / a_med, 3), algorithmic_gbs=round(algo / med / 1e6, 1),
                             fraction_of_8tbs=round(algo / med / 1e6 / HBM_PEAK_GBS, 4), moved_gbs=round(moved / med / 1e6, 1)))
            print("%-36s %9d AUs, %5d segments, GOP %2d: hbs_au_times %8.4f ms (min %8.4f), plan only %8.4f ms (min %8.4f); hbs_access_units %8.4f ms:"
                  " ratio %.3f; algorithmic %6.0f GB/s = %.4f of 8 TB/s, as built %6.0f GB/s"
                  % (batch, aus, int(s["nal_found"]), gop, med, lo, p_med, p_lo, a_med, med / a_med, algo / med / 1e6, algo / med / 1e6 / HBM_PEAK_GBS,
                     moved / med / 1e6), flush=True)

    # (a) config 3
    stream, n = stream_4k30(3, args.pictures)
    d = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).to(dev)
    idx, rbsp, summary, cap = ctx.alloc_outputs(d.numel(), index_cap=n + 16)
    ctx.index_extract_async(d, idx, cap, rbsp, summary)
    assert int(ctx.read_summary(summary)["nal_count"]) == n
    parsed = torch.empty(n * PARSED.itemsize, dtype=torch.uint8, device=dev)
    compact = torch.empty(n * COMPACT.itemsize, dtype=torch.uint8, device=dev)
    ps = torch.zeros(SUMMARY.itemsize, dtype=torch.uint8, device=dev)
    ctx.parse_compact_async(rbsp, idx, n, parsed, compact, None, ps)
    structs = torch.empty(int(ctx.read_summary(ps)["reserved"][0]) + 16, dtype=torch.uint8, device=dev)
    ctx.parse_compact_async(rbsp, idx, n, parsed, compact, structs, ps)
    assert int(ctx.read_summary(ps)["error"]) == 0
    a_med, a_lo, au, aus = access_units(idx, parsed, compact, structs, n)
    assert aus == args.pictures
    au_times("config 3 (4K30), %d NALs" % n, au, aus, a_med)
    del d, idx, rbsp, parsed, compact, structs, au
    torch.cuda.empty_cache()

    # (b) fabricated records: AUD, first slice, six more slices, suffix SEI... a picture every 8 NALs
    for n in [int(x) for x in args.nals.split(",") if x]:
        k = torch.arange(n, device=dev, dtype=torch.int64)
        ph = k % 8
        parsed = torch.zeros((n, 8), dtype=torch.int32, device=dev)            # rc, type, layer, tid1, struct_off (2), size, off
        parsed[:, 0] = 40
        parsed[:, 1] = torch.where(ph == 0, 35, torch.where(ph == 7, 40, 1)).to(torch.int32)
        parsed[:, 3] = 1
        parsed[:, 4] = -1
        parsed[:, 5] = -1
        compact = torch.zeros((n, 16), dtype=torch.int32, device=dev)
        compact[:, 0] = (ph == 1).to(torch.int32)
        compact[:, 5] = (k % 3).to(torch.int32)
        compact[:, 7] = ((k // 8) % 256).to(torch.int32)
        index = torch.zeros((n, 4), dtype=torch.int64, device=dev)
        index[:, 1] = (k + 1) * 128
        index[:, 0] = index[:, 1] - 120
        del k, ph
        a_med, a_lo, au, aus = access_units(index.view(torch.uint8).reshape(-1), parsed.view(torch.uint8).reshape(-1), compact.view(torch.uint8).reshape(-1), None, n)
        assert aus == (n + 7) // 8
        del parsed, compact, index
        torch.cuda.empty_cache()
        au_times("fabricated, %d NALs" % n, au, aus, a_med)
        del au
        torch.cuda.empty_cache()
    print(json.dumps({"autimes_time": rows, "source_digest": hbs.source_digest()}))


if __name__ == "__main__":
    main()
