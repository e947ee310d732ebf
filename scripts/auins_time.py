#!/usr/bin/env python3
"""Kernel time of hbs_au_insert (the library's HIP events around all of a call's launches, hbs_ctx_kernel_ms) on the bench stream
-- S(0x1234, n) of ~10 KiB NALs, 16 GiB by default, cut into access units of --au-nals NALs -- and on a stream of ~1 KiB NALs
(scripts/nal_sweep.py's shape, one NAL an AU, 2 GiB by default): AUDs only, the parameter sets in front of every 32nd AU
(flagged IRAP; the stream's first three NALs stand for the VPS, SPS and PPS), and both; all four output tables are written.
Next to them, in the same process, hbs_filter_annexb keeping everything on the same stream (output index written).  Traffic =
the bytes read + the bytes written of the stream and the output; the tables (per NAL 100 B read, 40 B written; per AU 128 B
read, 64 B written) and the scratch are not counted.  Fractions of the 8 TB/s peak.
    python scripts/auins_time.py [--gib 16] [--small-gib 2] [--reps 5] [--au-nals 8]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_PEAK_GBS = 8000.0
NONE = 0xFFFFFFFF


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

    def up(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)

    for name, stream, n, per in shapes():
        sb = stream.numel()
        ent, _, s = ctx.index_extract(stream, index_cap=n + 16, want_rbsp=False)
        assert len(ent) == n, (len(ent), n)
        ends = ent["end"].astype(np.uint64)
        k = np.arange(n, dtype=np.int64)
        parsed = np.zeros(n, dtype=hbs.PARSED)
        parsed["rc"], parsed["nal_unit_type"], parsed["nal_temporal_id_plus1"] = 1, np.where(k < 3, 32 + k, 1), 1
        n_aus = (n + per - 1) // per
        a = np.arange(n_aus, dtype=np.int64)
        au = np.zeros(n_aus, dtype=hbs.ACCESS_UNIT)
        au["first_nal"] = a * per
        au["nal_count"] = np.minimum(a * per + per, n) - a * per
        au["unit_end"] = ends[au["first_nal"] + au["nal_count"] - 1]
        au["unit_begin"][1:] = au["unit_end"][:-1]
        fv = np.maximum(3 - a * per, 0)
        pic = fv < au["nal_count"]
        au["first_vcl"] = np.where(pic, fv, NONE)
        au["vcl_count"] = np.where(pic, au["nal_count"] - fv, 0)
        au["nal_unit_type"], au["temporal_id_plus1"], au["slice_types"] = np.where(pic, 1, -1), np.where(pic, 1, 0), np.where(pic, 2, 0)
        au["flags"] = np.where(pic, np.where(a % 32 == 0, hbs.AU_IRAP, 0), hbs.AU_NO_PICTURE)
        nal_au = (k // per).astype(np.uint32)
        es_bytes = int(au["unit_end"][-1])
        d_idx, d_parsed, d_au, d_nal_au = up(ent), up(parsed), up(au), up(nal_au)
        del ent, parsed
        summ = torch.zeros(64, dtype=torch.uint8, device=dev)

        out = torch.empty(es_bytes + 16, dtype=torch.uint8, device=dev)
        io = torch.empty(n * 32, dtype=torch.uint8, device=dev)
        rule = ctx.nal_filter()

        def keep_all():
            ctx.filter_annexb_async(stream, sb, d_idx, n, out, io, summ, rule=rule, out_cap=es_bytes)
        f_ms = timed(keep_all)
        sm = ctx.read_summary(summ)
        assert int(sm["error"]) == 0 and int(sm["stream_bytes"]) == es_bytes and int(sm["nal_count"]) == n, sm
        f_med = f_ms[len(f_ms) // 2]
        results = [("hbs_filter_annexb, keep all", f_ms, es_bytes, es_bytes, 0, 0, None)]
        del out, io
        torch.cuda.empty_cache()

        for label, flags in (("AUD only", hbs.AUINS_AUD), ("sets at every 32nd AU", hbs.AUINS_PARAM_SETS), ("AUD and sets", hbs.AUINS_AUD | hbs.AUINS_PARAM_SETS)):
            ins = (stream, sb, d_idx, d_parsed, n, d_au, d_nal_au, n_aus, 0, n_aus, flags)
            assert ctx.au_insert_async(*ins, None, None, None, None, None, summ) == 0
            plan = ctx.read_summary(summ)
            assert int(plan["error"]) == 0, plan
            need, M = int(plan["stream_bytes"]), int(plan["nal_count"])
            out = torch.empty(need + 16, dtype=torch.uint8, device=dev)
            io = torch.empty(M * 32, dtype=torch.uint8, device=dev)
            src, nau = (torch.empty(M, dtype=torch.int32, device=dev) for _ in range(2))
            auo = torch.empty(n_aus * 64, dtype=torch.uint8, device=dev)

            def insert():
                assert ctx.au_insert_async(*ins, out, io, src, nau, auo, summ, out_cap=need, index_cap=M) == 0
            ms = timed(insert)
            sm = ctx.read_summary(summ)
            assert int(sm["error"]) == 0 and int(sm["stream_bytes"]) == need and int(sm["nal_count"]) == M, sm
            auds, sets = int(sm["reserved"][0]), int(sm["reserved"][1])
            # spot check, reported and not asserted: the scan of the output's first 64 MiB against d_index_out (but its cut last NAL)
            got, _, _ = ctx.index_extract(out[: min(need, 64 << 20)], want_rbsp=False)
            want = io[: max(len(got) - 1, 0) * 32].cpu().numpy().view(hbs.NAL_ENTRY)
            same = len(got) > 1 and bool(np.array_equal(got["start"][:-1], want["start"]) and np.array_equal(got["end"][:-1], want["end"]))
            results.append(("hbs_au_insert, " + label, ms, es_bytes + (need - es_bytes - 7 * auds - 4 * sets), need, auds, sets, same))
            del out, io, src, nau, auo
            torch.cuda.empty_cache()

        for call, ms, inb, outb, auds, sets, same in results:
            med = ms[len(ms) // 2]
            traffic = inb + outb
            row = dict(stream=name, call=call, nals=n, aus=n_aus, auds=auds, sets=sets, head_rescan_matches=same, in_bytes=inb, out_bytes=outb, kernel_ms_min=round(ms[0], 4),
                       kernel_ms_median=round(med, 4), traffic_bytes=traffic, gbs=round(traffic / med / 1e6, 1),
                       fraction_of_8tbs=round(traffic / med / 1e6 / HBM_PEAK_GBS, 3), time_over_filter=round(med / f_med, 3))
            rows.append(row)
            print("%-44s %-40s %8.3f ms (min %8.3f)  %6.2f GiB in  %6.2f GiB out  %7.0f GB/s  %.3f of 8 TB/s (bytes read + bytes written)  %.3f x the filter's time"
                  % (name, call, med, ms[0], inb / 2**30, outb / 2**30, row["gbs"], row["fraction_of_8tbs"], row["time_over_filter"]), flush=True)
        del stream, d_idx, d_parsed, d_au, d_nal_au
        torch.cuda.empty_cache()
    print(json.dumps({"auins_time": rows, "source_digest": hbs.source_digest()}))


if __name__ == "__main__":
    main()
