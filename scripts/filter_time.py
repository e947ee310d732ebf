#!/usr/bin/env python3
"""Kernel time of hbs_filter_annexb (the library's HIP events around all of a call's launches, hbs_ctx_kernel_ms) on the bench
stream -- S(0x1234, n) of ~10 KiB NALs, 16 GiB by default -- and on streams of ~1 KiB and ~128-byte NALs (scripts/nal_sweep.py's
shape, 2 GiB by default).  Three cuts each: keep-all (a rule), every other NAL (d_keep) and ~10 % of the NALs (d_keep).
Traffic from the shapes: the kept units read and written, the index read twice (32 B a NAL), d_keep read twice (1 B a NAL),
32 B of output index a kept NAL, 16 B of scratch a kept unit written and read back; fraction of the 8 TB/s peak.
    python scripts/filter_time.py [--gib 16] [--small-gib 2] [--reps 5]"""
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

    for name, stream, n in shapes():
        sb = stream.numel()
        ent, _, s = ctx.index_extract(stream, index_cap=n + 16, want_rbsp=False)
        assert len(ent) == n, (len(ent), n)
        d_idx = torch.from_numpy(ent.view(np.uint8).copy()).to(dev)
        en = ent["end"].astype(np.int64)
        unit = en - np.concatenate([[0], en[:-1]])
        out = torch.empty(sb + 16, dtype=torch.uint8, device=dev)
        io = torch.empty(n * 32, dtype=torch.uint8, device=dev)
        summ = torch.zeros(64, dtype=torch.uint8, device=dev)
        rng = np.random.RandomState(1)
        cuts = [("keep-all (rule)", None), ("every other NAL (d_keep)", np.arange(n) % 2 == 0),
                ("~10 % of the NALs (d_keep)", rng.rand(n) < 0.1)]
        for cut, keep in cuts:
            d_keep = None if keep is None else torch.from_numpy(keep.astype(np.uint8)).to(dev)
            rule = ctx.nal_filter() if keep is None else None
            kmask = np.ones(n, bool) if keep is None else keep
            ctx.enable_timing(True)
            ctx.filter_annexb_async(stream, sb, d_idx, n, out, io, summ, rule=rule, keep=d_keep)     # warm-up
            for _ in range(args.reps):
                ctx.filter_annexb_async(stream, sb, d_idx, n, out, io, summ, rule=rule, keep=d_keep)
            ms = sorted(ctx.kernel_ms_back(b) for b in range(args.reps))
            ctx.enable_timing(False)
            sm = ctx.read_summary(summ)
            assert int(sm["error"]) == 0, sm
            ob = int(sm["stream_bytes"])
            assert ob == int(unit[kmask].sum())
            if keep is None:
                assert torch.equal(out[:ob], stream[:ob])
            kept = int(kmask.sum())
            traffic = 2 * ob + 64 * n + (2 * n if keep is not None else 0) + 32 * kept + 32 * int((unit[kmask] > 0).sum())
            med = ms[len(ms) // 2]
            row = dict(stream=name, stream_bytes=sb, nals=n, cut=cut, kept_nals=kept, out_bytes=ob,
                       kernel_ms_min=round(ms[0], 4), kernel_ms_median=round(med, 4), traffic_bytes=traffic,
                       gbs=round(traffic / med / 1e6, 1), fraction_of_8tbs=round(traffic / med / 1e6 / HBM_PEAK_GBS, 3))
            rows.append(row)
            print("%-34s %-28s %8.3f ms (min %8.3f)  %6.2f GiB out  %7.0f GB/s  %.3f of 8 TB/s"
                  % (name, row["cut"], med, ms[0], ob / 2**30, row["gbs"], row["fraction_of_8tbs"]), flush=True)
        del out, io, d_idx, stream
        torch.cuda.empty_cache()
    print(json.dumps({"filter_time": rows, "source_digest": hbs.source_digest()}))


if __name__ == "__main__":
    main()
