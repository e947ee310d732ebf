#!/usr/bin/env python3
"""Kernel time of hbs_mp4_stbl_write (the library's HIP events around all of a call's launches, hbs_ctx_kernel_ms) for the two
README shapes: the bench stream S(0x1234, n) of ~10 KiB NALs, 16 GiB by default, AUs of --au-nals NALs; and ~1 KiB NALs, one an
AU, 2 GiB by default.  The sample tables are those hbs_mp4_fragment writes (cut at every 32nd AU, so the samples lie in
stretches of 32 with a moof between them and the chunks come out 32 long).  Rows: offsets and sizes alone (no d_dts: an stts of
one entry), and with d_dts, d_pts (a ctts of an entry a sample) and d_sample_flags (every 32nd a sync sample); each plan only and
in full; once more with max_chunk_samples = 8.  Next to it, in the same process: hbs_mp4_stbl_samples reading back the boxes
just written, with the record d_tables gave, which must return the tables that went in.
    python scripts/mp4stblw_time.py [--gib 16] [--small-gib 2] [--reps 5] [--au-nals 8]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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
        yield ("S(0x1234, %d) ~10 KiB NALs, AUs of %d NALs" % (n, args.au_nals), g["stream"][: g["stream_bytes"]], n, args.au_nals)
        del g
        arena, total, idx, n, stream, sb = make_stream(torch, np, ctx, 1024, int(args.small_gib * 2**30))
        del arena, idx
        yield ("random payload, AUs of one ~1 KiB NAL", stream[:sb], n, 1)

    def timed(call, reps):
        ctx.enable_timing(True)
        call()                                          # warm-up
        for _ in range(reps):
            call()
        ms = sorted(ctx.kernel_ms_back(b) for b in range(reps))
        ctx.enable_timing(False)
        return ms

    def up(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)

    for name, stream, n, per in shapes():
        sb = stream.numel()
        ent, _, s = ctx.index_extract(stream, index_cap=n + 16, want_rbsp=False)
        assert len(ent) == n, (len(ent), n)
        n_aus = (n + per - 1) // per
        au = np.zeros(n_aus, dtype=hbs.ACCESS_UNIT)
        au["flags"] = np.where(np.arange(n_aus) % 32 == 0, hbs.AU_IRAP, 0)
        nal_au = (np.arange(n, dtype=np.int64) // per).astype(np.uint32)
        d_idx, d_au, d_nal_au = up(ent), up(au), up(nal_au)
        del ent
        summ = torch.zeros(64, dtype=torch.uint8, device=dev)
        prm = hbs.mp4_params(length_size=4, track_id=1, sequence=1, sample_duration=3003, flags=hbs.MP4_CUT_AT_IRAP)
        a = (stream, sb, d_idx, n, d_nal_au, d_au, n_aus, prm)
        assert ctx.mp4_fragment_async(*a, None, summ) == 0
        plan = ctx.read_summary(summ)
        assert int(plan["error"]) == 0, plan
        need, frags = int(plan["stream_bytes"]), int(plan["nal_count"])
        out = torch.empty(need + 16, dtype=torch.uint8, device=dev)
        so, ss = (torch.empty(n_aus * 8, dtype=torch.uint8, device=dev) for _ in range(2))
        assert ctx.mp4_fragment_async(*a, out, summ, sample_off=so, sample_size=ss, out_cap=need) == 0
        assert int(ctx.read_summary(summ)["error"]) == 0
        del out, d_idx, d_au, d_nal_au
        torch.cuda.empty_cache()
        chunks = (n_aus + 31) // 32
        k = np.arange(n_aus, dtype=np.uint64)
        dts = k * np.uint64(3003)
        d_dts, d_pts = up(dts), up(dts + np.uint64(3003) * (k % np.uint64(3)))
        d_fl = up(np.where(k % 32 == 0, 0x02000000, 0x01010000).astype(np.uint32))
        co64 = hbs.MP4_STBL_CO64 if need >= 1 << 32 else 0
        cap = hbs.mp4_stbl_write_bytes(n_aus, True, True, co64)
        boxes = torch.empty(cap, dtype=torch.uint8, device=dev)
        rec = torch.zeros(hbs.MP4_STBL.itemsize, dtype=torch.uint8, device=dev)
        t_off, t_size, t_dts, t_pts = (torch.empty(n_aus * 8, dtype=torch.uint8, device=dev) for _ in range(4))
        t_fl = torch.empty(n_aus * 4, dtype=torch.uint8, device=dev)
        results = []
        for label, times, m in (("offsets and sizes alone", False, 0), ("with d_dts, d_pts (a ctts entry a sample), d_sample_flags", True, 0),
                                ("the same with max_chunk_samples 8", True, 8)):
            wp = hbs.mp4_stbl_write_params(flags=co64, max_chunk_samples=m, sample_duration=3003, data_offset=48)
            kw = dict(dts=d_dts, pts=d_pts, sample_flags=d_fl) if times else {}
            want_chunks = chunks if not m else int(np.sum((np.minimum(n_aus - np.arange(0, n_aus, 32), 32) + m - 1) // m))

            def planned():
                assert ctx.mp4_stbl_write_async(so, ss, n_aus, wp, summ, **kw) == 0

            def full():
                assert ctx.mp4_stbl_write_async(so, ss, n_aus, wp, summ, out=boxes, out_cap=cap, tables=rec, **kw) == 0
            for what, call in (("plan only", planned), ("in full", full)):
                ms = timed(call, args.reps)
                sm = ctx.read_summary(summ)
                same = int(sm["error"]) == 0 and int(sm["nal_count"]) == n_aus and int(sm["nal_found"]) == want_chunks
                results.append(("hbs_mp4_stbl_write, %s, %s" % (label, what), ms, same, int(sm["stream_bytes"])))
            # the reader next to it, on what was just written
            T = int(ctx.read_summary(summ)["stream_bytes"])
            tables = rec.cpu().numpy().view(hbs.MP4_STBL).copy()
            tables["file_bytes"] = need + 48
            outs = dict(sample_off=t_off, sample_size=t_size, dts=t_dts, pts=t_pts, sample_flags=t_fl)

            def read_back():
                assert ctx.mp4_stbl_samples_async(boxes, T, tables, summ, sample_cap=n_aus, **outs) == 0
            ms = timed(read_back, args.reps)
            sm = ctx.read_summary(summ)
            same = (int(sm["error"]) == 0 and int(sm["nal_count"]) == n_aus and bool(torch.equal(t_size, ss))
                    and bool(torch.equal(t_off.view(torch.int64), so.view(torch.int64) + 48)))
            if times:
                same = same and bool(torch.equal(t_dts, d_dts)) and bool(torch.equal(t_pts, d_pts))
                same = same and bool(torch.equal(t_fl.view(torch.int32) != 0, (d_fl.view(torch.int32) & 0x00010000) != 0))
            results.append(("hbs_mp4_stbl_samples reading those boxes back, " + label, ms, same, T))

        for call, ms, same, T in results:
            med = ms[len(ms) // 2]
            row = dict(stream=name, call=call, samples=n_aus, box_bytes=T, agrees=same, kernel_ms_min=round(ms[0], 4), kernel_ms_median=round(med, 4),
                       kernel_ms_max=round(ms[-1], 4), repeats=len(ms), ns_per_sample=round(med * 1e6 / max(n_aus, 1), 2))
            rows.append(row)
            print("%-44s %-100s %9.3f ms (min %9.3f, max %9.3f of %d)  %8d samples %10d box bytes  %7.2f ns a sample  %s"
                  % (name, call, med, ms[0], ms[-1], len(ms), n_aus, T, row["ns_per_sample"], "agrees" if same else "DIFFERS"), flush=True)
        del stream, so, ss, boxes, d_dts, d_pts, d_fl, t_off, t_size, t_dts, t_pts, t_fl
        torch.cuda.empty_cache()
    print(json.dumps({"mp4stblw_time": rows, "source_digest": hbs.source_digest()}))


if __name__ == "__main__":
    main()
