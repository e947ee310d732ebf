#!/usr/bin/env python3
"""Kernel time of hbs_access_units (the library's HIP events around all of a call's launches, hbs_ctx_kernel_ms; median of
--reps calls after a warm-up, one process):
  (a) on BASELINE config 3's 4K30 stream (100 627 NALs), next to hbs_parse_headers_compact on the same batch; the parse records
      none of the library's events, so both are also measured with events of the stream around each call;
  (b) on fabricated records with a picture every 8 NALs, as a fraction of the 8 TB/s peak.  Algorithmic bytes: 96 B a NAL of
      records read, 4 B a NAL of d_nal_au and 64 B an AU written; the call as built moves more -- a 16-byte digest a NAL written
      once and read three times, 4 B of it rewritten -- and that figure is printed next to it.
    python scripts/au_time.py [--reps 21] [--nals 16777216,134217728] [--pictures 12500]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_PEAK_GBS = 8000.0


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

    def timed_stream(call):
        """the same with events of the caller's stream around each call (the parse records none of the library's own)"""
        call()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        for a, b in ev:
            a.record()
            call()
            b.record()
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in ev)
        return ms[len(ms) // 2], ms[0]

    def au_call(index, parsed, compact, structs, n):
        summ = torch.zeros(SUMMARY.itemsize, dtype=torch.uint8, device=dev)
        assert ctx.access_units_async(index, parsed, compact, structs, n, None, 0, None, None, summ) == 0
        aus = int(ctx.read_summary(summ)["nal_count"])
        au = torch.empty(max(aus, 1) * ACCESS_UNIT.itemsize, dtype=torch.uint8, device=dev)
        nal_au = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        carry = torch.zeros(16, dtype=torch.uint8, device=dev)
        med, lo = timed(lambda: ctx.access_units_async(index, parsed, compact, structs, n, au, aus, nal_au, carry, summ))
        sm = ctx.read_summary(summ)
        assert int(sm["error"]) == 0 and int(sm["nal_count"]) == aus
        au_call.stream_ms = timed_stream(lambda: ctx.access_units_async(index, parsed, compact, structs, n, au, aus, nal_au, carry, summ))
        return med, lo, aus, int(sm["reserved"][0])

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
    p_med, p_lo = timed_stream(lambda: ctx.parse_compact_async(rbsp, idx, n, parsed, compact, structs, ps))
    assert int(ctx.read_summary(ps)["error"]) == 0
    a_med, a_lo, aus, pics = au_call(idx, parsed, compact, structs, n)
    assert aus == pics == args.pictures
    s_med, s_lo = au_call.stream_ms
    rows.append(dict(batch="config 3 (4K30)", nals=n, aus=aus, parse_compact_stream_ms_median=round(p_med, 4), parse_compact_stream_ms_min=round(p_lo, 4),
                     access_units_stream_ms_median=round(s_med, 4), access_units_stream_ms_min=round(s_lo, 4),
                     access_units_ms_median=round(a_med, 4), access_units_ms_min=round(a_lo, 4), ratio=round(s_med / p_med, 3)))
    print("config 3: %d NALs, %d AUs, events of the stream around each call: hbs_parse_headers_compact %.4f ms (min %.4f), hbs_access_units %.4f ms (min %.4f)"
          " = %.2f of the parse; the library's own events around hbs_access_units' launches: %.4f ms (min %.4f)"
          % (n, aus, p_med, p_lo, s_med, s_lo, s_med / p_med, a_med, a_lo), flush=True)
    del d, idx, rbsp, parsed, compact, structs
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
        med, lo, aus, pics = au_call(index.view(torch.uint8).reshape(-1), parsed.view(torch.uint8).reshape(-1), compact.view(torch.uint8).reshape(-1), None, n)
        assert aus == pics == (n + 7) // 8
        algo = 96 * n + 4 * n + 64 * aus
        moved = algo + (16 + 3 * 16 + 4) * n
        rows.append(dict(batch="fabricated, a picture every 8 NALs", nals=n, aus=aus, access_units_ms_median=round(med, 4), access_units_ms_min=round(lo, 4),
                         algorithmic_bytes=algo, algorithmic_gbs=round(algo / med / 1e6, 1), fraction_of_8tbs=round(algo / med / 1e6 / HBM_PEAK_GBS, 3),
                         moved_bytes=moved, moved_gbs=round(moved / med / 1e6, 1), moved_fraction_of_8tbs=round(moved / med / 1e6 / HBM_PEAK_GBS, 3)))
        print("fabricated %11d NALs, %9d AUs: %9.4f ms (min %9.4f)  algorithmic %6.0f GB/s = %.3f of 8 TB/s; as built (digest passes) %6.0f GB/s = %.3f"
              % (n, aus, med, lo, algo / med / 1e6, algo / med / 1e6 / HBM_PEAK_GBS, moved / med / 1e6, moved / med / 1e6 / HBM_PEAK_GBS), flush=True)
        del parsed, compact, index
        torch.cuda.empty_cache()
    print(json.dumps({"au_time": rows, "source_digest": hbs.source_digest()}))


if __name__ == "__main__":
    main()
