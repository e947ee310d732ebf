#!/usr/bin/env python3
"""Kernel time of hbs_mp4_fragment (the library's HIP events around all of a call's launches, hbs_ctx_kernel_ms), all tables
written, on the bench stream -- S(0x1234, n) of ~10 KiB NALs, 16 GiB by default, cut into access units of --au-nals NALs, an
IRAP every 32nd AU, HBS_MP4_CUT_AT_IRAP -- and on a stream of ~1 KiB NALs (scripts/nal_sweep.py's shape, one NAL an AU, 2 GiB by
default) two ways: HBS_MP4_CUT_AT_IRAP every 32, and max_samples 1 (a moof in front of every sample: the header-heavy worst
case).  Next to each row, in the same process, hbs_annexb_to_lenpref with its sample table on the same stream: the copy this
call replaces.  Traffic = the NAL bytes read + the output bytes written; the tables (per NAL 36 B read; per AU 64 B read, 16 B
written) and the scratch are not counted.  Fractions of the 8 TB/s peak.
    python scripts/mp4_time.py [--gib 16] [--small-gib 2] [--reps 5] [--au-nals 8]"""
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
        yield ("S(0x1234, %d) ~10 KiB NALs, AUs of %d NALs" % (n, args.au_nals), g["stream"][: g["stream_bytes"]], n, args.au_nals,
               (("cut at every 32nd AU", dict(flags=hbs.MP4_CUT_AT_IRAP)),))
        del g
        arena, total, idx, n, stream, sb = make_stream(torch, np, ctx, 1024, int(args.small_gib * 2**30))
        del arena, idx
        yield ("random payload, AUs of one ~1 KiB NAL", stream[:sb], n, 1,
               (("cut at every 32nd AU", dict(flags=hbs.MP4_CUT_AT_IRAP)), ("max_samples 1", dict(max_samples=1))))

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

    for name, stream, n, per, modes in shapes():
        sb = stream.numel()
        ent, _, s = ctx.index_extract(stream, index_cap=n + 16, want_rbsp=False)
        assert len(ent) == n, (len(ent), n)
        nal_bytes = int((ent["end"] - ent["start"]).sum())
        n_aus = (n + per - 1) // per
        au = np.zeros(n_aus, dtype=hbs.ACCESS_UNIT)
        au["flags"] = np.where(np.arange(n_aus) % 32 == 0, hbs.AU_IRAP, 0)
        nal_au = (np.arange(n, dtype=np.int64) // per).astype(np.uint32)
        d_idx, d_au, d_nal_au = up(ent), up(au), up(nal_au)
        del ent
        summ = torch.zeros(64, dtype=torch.uint8, device=dev)

        rec = nal_bytes + 4 * n
        out = torch.empty(rec + 16, dtype=torch.uint8, device=dev)
        so = torch.empty((n_aus + 1) * 8, dtype=torch.uint8, device=dev)

        def lenpref():
            ctx.annexb_to_lenpref_async(stream, sb, d_idx, n, out, None, summ, length_size=4, nal_au=d_nal_au, n_aus=n_aus, sample_off=so, out_cap=rec)
        l_ms = timed(lenpref)
        sm = ctx.read_summary(summ)
        assert int(sm["error"]) == 0 and int(sm["stream_bytes"]) == rec and int(sm["nal_count"]) == n, sm
        l_med = l_ms[len(l_ms) // 2]
        results = [("hbs_annexb_to_lenpref, sample table", l_ms, rec, 0, None)]
        del out, so
        torch.cuda.empty_cache()

        for label, kw in modes:
            prm = hbs.mp4_params(length_size=4, track_id=1, sequence=1, sample_duration=3003, **kw)
            a = (stream, sb, d_idx, n, d_nal_au, d_au, n_aus, prm)
            assert ctx.mp4_fragment_async(*a, None, summ) == 0
            plan = ctx.read_summary(summ)
            assert int(plan["error"]) == 0, plan
            need, frags = int(plan["stream_bytes"]), int(plan["nal_count"])
            assert need == rec + 16 * n_aus + 96 * frags
            out = torch.empty(need + 16, dtype=torch.uint8, device=dev)
            so, ss = (torch.empty(n_aus * 8, dtype=torch.uint8, device=dev) for _ in range(2))
            fr = torch.empty(frags * hbs.MP4_FRAG.itemsize, dtype=torch.uint8, device=dev)

            def fragment():
                assert ctx.mp4_fragment_async(*a, out, summ, sample_off=so, sample_size=ss, frag=fr, frag_cap=frags, out_cap=need) == 0
            ms = timed(fragment)
            sm = ctx.read_summary(summ)
            assert int(sm["error"]) == 0 and int(sm["stream_bytes"]) == need and int(sm["nal_count"]) == frags, sm
            # spot check, reported and not asserted: the first fragment's boxes, and its first sample against the stream
            f0 = fr[: hbs.MP4_FRAG.itemsize].cpu().numpy().view(hbs.MP4_FRAG)[0]
            head = out[:8].cpu().numpy().tobytes()
            s0, z0 = int(so[:8].cpu().numpy().view(np.uint64)[0]), int(ss[:8].cpu().numpy().view(np.uint64)[0])
            e0 = d_idx[:32].cpu().numpy().view(hbs.NAL_ENTRY)[0]
            w = min(int(e0["end"] - e0["start"]), 4096)
            same = (head[4:] == b"moof" and int.from_bytes(head[:4], "big") == 88 + 16 * int(f0["samples"]) and s0 == 96 + 16 * int(f0["samples"])
                    and z0 > 0 and bool(torch.equal(out[s0 + 4: s0 + 4 + w], stream[int(e0["start"]): int(e0["start"]) + w])))
            results.append(("hbs_mp4_fragment, " + label, ms, need, frags, same))
            del out, so, ss, fr
            torch.cuda.empty_cache()

        for call, ms, outb, frags, same in results:
            med = ms[len(ms) // 2]
            traffic = nal_bytes + outb
            row = dict(stream=name, call=call, nals=n, aus=n_aus, fragments=frags, first_fragment_checks=same, in_bytes=nal_bytes, out_bytes=outb,
                       kernel_ms_min=round(ms[0], 4), kernel_ms_median=round(med, 4), traffic_bytes=traffic, gbs=round(traffic / med / 1e6, 1),
                       fraction_of_8tbs=round(traffic / med / 1e6 / HBM_PEAK_GBS, 3), time_over_lenpref=round(med / l_med, 3))
            rows.append(row)
            print("%-44s %-40s %8.3f ms (min %8.3f)  %6.2f GiB in  %6.2f GiB out  %8d fragments  %7.0f GB/s  %.3f of 8 TB/s (NAL bytes read + output written)  %.3f x the length-prefix call's time"
                  % (name, call, med, ms[0], nal_bytes / 2**30, outb / 2**30, frags, row["gbs"], row["fraction_of_8tbs"], row["time_over_lenpref"]), flush=True)
        del stream, d_idx, d_au, d_nal_au
        torch.cuda.empty_cache()
    print(json.dumps({"mp4_time": rows, "source_digest": hbs.source_digest()}))


if __name__ == "__main__":
    main()
