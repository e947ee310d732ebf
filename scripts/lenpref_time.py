#!/usr/bin/env python3
"""Kernel time of hbs_annexb_to_lenpref and hbs_lenpref_to_annexb (the library's HIP events around all of a call's launches,
hbs_ctx_kernel_ms) on the bench stream -- S(0x1234, n) of ~10 KiB NALs, 16 GiB by default -- and on streams of ~1 KiB and
~128-byte NALs (scripts/nal_sweep.py's shape, 2 GiB by default): keep-all, length_size 4, 4-byte start codes, samples of
--au-nals NALs each.  In the same process, on the same stream: hbs_filter_annexb keep-all, the nearest existing copy.
Traffic from the shapes.  Forward: the payloads read and written, 4 B a NAL of length fields written, the index read twice
(32 B a NAL), 32 B of output index a NAL, 16 B of scratch a NAL written and read back, the AU numbers read twice (4 B a NAL),
8 B a sample.  Reverse: the payloads read and written, the length fields read twice (4 B a NAL), 4 B a NAL of start codes
written, 16 B of scratch a NAL written and read back, 16 B a sample of table read twice, 16 B a sample of scratch written and
read back, 8 B a sample written.  The filter: as scripts/filter_time.py.  Fractions of the 8 TB/s peak.
    python scripts/lenpref_time.py [--gib 16] [--small-gib 2] [--reps 5] [--au-nals 8]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_PEAK_GBS = 8000.0


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
        yield "S(0x1234, %d) ~10 KiB NALs" % n, g["stream"][: g["stream_bytes"]], n
        del g
        for mean in (1024, 128):
            arena, total, idx, n, stream, sb = make_stream(torch, np, ctx, mean, int(args.small_gib * 2**30))
            del arena, idx
            yield "random payload, ~%d-byte NALs" % mean, stream[:sb], n

    def timed(call):
        ctx.enable_timing(True)
        call()                                          # warm-up
        for _ in range(args.reps):
            call()
        ms = sorted(ctx.kernel_ms_back(b) for b in range(args.reps))
        ctx.enable_timing(False)
        return ms

    for name, stream, n in shapes():
        sb = stream.numel()
        ent, _, s = ctx.index_extract(stream, index_cap=n + 16, want_rbsp=False)
        assert len(ent) == n, (len(ent), n)
        d_idx = torch.from_numpy(ent.view(np.uint8).copy()).to(dev)
        pay = int((ent["end"] - ent["start"]).astype(np.int64).sum())
        unit_bytes = int(ent["end"][-1])
        n_aus = (n + args.au_nals - 1) // args.au_nals
        d_au = (torch.arange(n, device=dev, dtype=torch.int64) // args.au_nals).to(torch.int32)
        rec_bytes = pay + 4 * n
        rec = torch.empty(rec_bytes + 16, dtype=torch.uint8, device=dev)
        back = torch.empty(max(rec_bytes, sb) + 16, dtype=torch.uint8, device=dev)
        io = torch.empty(n * 32, dtype=torch.uint8, device=dev)
        so = torch.empty((n_aus + 1) * 8, dtype=torch.uint8, device=dev)
        so2 = torch.empty((n_aus + 1) * 8, dtype=torch.uint8, device=dev)
        summ = torch.zeros(64, dtype=torch.uint8, device=dev)
        results = {}

        def fwd():
            assert ctx.annexb_to_lenpref_async(stream, sb, d_idx, n, rec, io, summ, length_size=4, nal_au=d_au, n_aus=n_aus,
                                               sample_off=so, out_cap=rec_bytes) == 0
        ms = timed(fwd)
        sm = ctx.read_summary(summ)
        assert int(sm["error"]) == 0 and int(sm["stream_bytes"]) == rec_bytes and int(sm["nal_count"]) == n, sm
        results["annexb_to_lenpref"] = (ms, 2 * pay + 4 * n + 64 * n + 32 * n + 32 * n + 8 * n + 8 * n_aus, rec_bytes)
        sample_off = so.view(torch.int64)
        size = (sample_off[1:] - sample_off[:-1]).contiguous()

        def rev():
            assert ctx.lenpref_to_annexb_async(rec, rec_bytes, so, size, n_aus, back, so2, summ, length_size=4, startcode_bytes=4,
                                               nal_cap=n, out_cap=rec_bytes) == 0
        ms = timed(rev)
        sm = ctx.read_summary(summ)
        assert int(sm["error"]) == 0 and int(sm["stream_bytes"]) == rec_bytes and int(sm["nal_count"]) == n, sm
        assert torch.equal(so2, so)                     # L equals the start code's size: the samples stay where they were
        results["lenpref_to_annexb"] = (ms, 2 * pay + 8 * n + 4 * n + 32 * n + 32 * n_aus + 32 * n_aus + 8 * n_aus, rec_bytes)
        got, _, _ = ctx.index_extract(back[:rec_bytes], index_cap=n + 16, want_rbsp=False)
        assert len(got) == n and np.array_equal(got["end"] - got["start"], ent["end"] - ent["start"])

        rule = ctx.nal_filter()

        def flt():
            ctx.filter_annexb_async(stream, sb, d_idx, n, back, io, summ, rule=rule, out_cap=sb)
        ms = timed(flt)
        sm = ctx.read_summary(summ)
        assert int(sm["error"]) == 0 and int(sm["stream_bytes"]) == unit_bytes, sm
        results["filter_annexb keep-all"] = (ms, 2 * unit_bytes + 64 * n + 32 * n + 32 * n, unit_bytes)

        f_med = results["filter_annexb keep-all"][0][args.reps // 2]
        for call, (ms, traffic, ob) in results.items():
            med = ms[len(ms) // 2]
            row = dict(stream=name, stream_bytes=sb, nals=n, samples=n_aus, call=call, out_bytes=ob, kernel_ms_min=round(ms[0], 4),
                       kernel_ms_median=round(med, 4), traffic_bytes=traffic, gbs=round(traffic / med / 1e6, 1),
                       fraction_of_8tbs=round(traffic / med / 1e6 / HBM_PEAK_GBS, 3), time_over_filter=round(med / f_med, 3))
            rows.append(row)
            print("%-34s %-24s %8.3f ms (min %8.3f)  %6.2f GiB out  %7.0f GB/s  %.3f of 8 TB/s  %.3f x the filter's time"
                  % (name, call, med, ms[0], ob / 2**30, row["gbs"], row["fraction_of_8tbs"], row["time_over_filter"]), flush=True)
        del rec, back, io, d_idx, stream, so, so2
        torch.cuda.empty_cache()
    print(json.dumps({"lenpref_time": rows, "source_digest": hbs.source_digest()}))


if __name__ == "__main__":
    main()
