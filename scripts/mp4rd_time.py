#!/usr/bin/env python3
"""Kernel time of hbs_mp4_samples (the library's HIP events around all of a call's launches, hbs_ctx_kernel_ms), all five tables
and d_frag written, on the output of hbs_mp4_fragment for the three shapes of scripts/mp4_time.py: the bench stream S(0x1234, n)
of ~10 KiB NALs, 16 GiB by default, AUs of --au-nals NALs cut at every 32nd AU; ~1 KiB NALs, one an AU, 2 GiB by default, cut at
every 32nd AU; and the same with max_samples 1 (a moof in front of every sample).  Each shape twice: the fragment table of
hbs_mp4_fragment passed as the segments at stride 48 (a lane a fragment), and the buffer as ONE segment (one lane walks the
whole chain, a dependent load a box; on at most --chain-frags fragments of the buffer, since the time is the chain's).  Next to
them, in the same process and on the same data: hbs_mp4_fragment that wrote the buffer, and hbs_lenpref_to_annexb that reads
the samples the table names.
    python scripts/mp4rd_time.py [--gib 16] [--small-gib 2] [--reps 5] [--au-nals 8] [--chain-frags 65536]"""
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
    ap.add_argument("--chain-frags", type=int, default=65536)
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

    for name, stream, n, per, modes in shapes():
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
        for label, kw in modes:
            prm = hbs.mp4_params(length_size=4, track_id=1, sequence=1, sample_duration=3003, **kw)
            a = (stream, sb, d_idx, n, d_nal_au, d_au, n_aus, prm)
            assert ctx.mp4_fragment_async(*a, None, summ) == 0
            plan = ctx.read_summary(summ)
            assert int(plan["error"]) == 0, plan
            need, frags = int(plan["stream_bytes"]), int(plan["nal_count"])
            out = torch.empty(need + 16, dtype=torch.uint8, device=dev)
            so, ss = (torch.empty(n_aus * 8, dtype=torch.uint8, device=dev) for _ in range(2))
            fr = torch.empty(frags * hbs.MP4_FRAG.itemsize, dtype=torch.uint8, device=dev)

            def fragment():
                assert ctx.mp4_fragment_async(*a, out, summ, sample_off=so, sample_size=ss, frag=fr, frag_cap=frags, out_cap=need) == 0
            results = [("hbs_mp4_fragment", timed(fragment, args.reps), frags, n_aus, None)]
            assert int(ctx.read_summary(summ)["error"]) == 0

            rp = hbs.mp4_read_params(track_id=1)
            t_off, t_size, t_dts, t_pts = (torch.empty(n_aus * 8, dtype=torch.uint8, device=dev) for _ in range(4))
            t_fl = torch.empty(n_aus * 4, dtype=torch.uint8, device=dev)
            t_fr = torch.empty(frags * hbs.MP4_FRAG.itemsize, dtype=torch.uint8, device=dev)
            tables = dict(sample_off=t_off, sample_size=t_size, dts=t_dts, pts=t_pts, sample_flags=t_fl, frag=t_fr)

            def by_table():
                assert ctx.mp4_samples_async(out, need, rp, summ, seg=fr, seg_stride=hbs.MP4_FRAG.itemsize, n_segs=frags, moof_cap=frags,
                                             sample_cap=n_aus, **tables) == 0
            ms = timed(by_table, args.reps)
            sm = ctx.read_summary(summ)
            same = (int(sm["error"]) == 0 and int(sm["nal_count"]) == n_aus and int(sm["nal_found"]) == frags
                    and bool(torch.equal(t_off, so)) and bool(torch.equal(t_size, ss)) and bool(torch.equal(t_fr, fr)))
            results.append(("hbs_mp4_samples, fragment table as segments (stride 48)", ms, frags, n_aus, same))

            def plan_only():
                assert ctx.mp4_samples_async(out, need, rp, summ, seg=fr, seg_stride=hbs.MP4_FRAG.itemsize, n_segs=frags, moof_cap=frags) == 0
            ms = timed(plan_only, args.reps)
            sm = ctx.read_summary(summ)
            same = int(sm["error"]) == 0 and int(sm["nal_count"]) == n_aus and int(sm["nal_found"]) == frags
            results.append(("hbs_mp4_samples, plan only (a lane a moof over its entries), same segments", ms, frags, n_aus, same))

            # one segment: the first `cf` fragments of the buffer
            cf = min(frags, args.chain_frags)
            f_host = fr.cpu().numpy().view(hbs.MP4_FRAG)
            cut = need if cf == frags else int(f_host["out_off"][cf])
            cs = n_aus if cf == frags else int(f_host["first_au"][cf])

            def one_segment():
                assert ctx.mp4_samples_async(out, cut, rp, summ, moof_cap=cf, sample_cap=cs, **tables) == 0
            ms = timed(one_segment, min(args.reps, 2))
            sm = ctx.read_summary(summ)
            same = (int(sm["error"]) == 0 and int(sm["nal_count"]) == cs and int(sm["nal_found"]) == cf
                    and bool(torch.equal(t_off[: cs * 8], so[: cs * 8])) and bool(torch.equal(t_size[: cs * 8], ss[: cs * 8])))
            results.append(("hbs_mp4_samples, one segment (%d fragments, %d boxes)" % (cf, 2 * cf), ms, cf, cs, same))
            del t_dts, t_pts, t_fl, t_fr

            # the copy the table feeds
            assert ctx.lenpref_to_annexb_async(out, need, t_off, t_size, n_aus, None, None, summ, length_size=4, startcode_bytes=4, nal_cap=1 << 62) == 0
            lp = ctx.read_summary(summ)
            assert int(lp["error"]) == 0, lp
            back_bytes, recs = int(lp["stream_bytes"]), int(lp["nal_count"])
            back = torch.empty(back_bytes + 16, dtype=torch.uint8, device=dev)

            def annexb():
                assert ctx.lenpref_to_annexb_async(out, need, t_off, t_size, n_aus, back, None, summ, length_size=4, startcode_bytes=4,
                                                   nal_cap=recs, out_cap=back_bytes) == 0
            results.append(("hbs_lenpref_to_annexb on that table", timed(annexb, args.reps), frags, n_aus, int(ctx.read_summary(summ)["error"]) == 0))
            del back, out, so, ss, fr, t_off, t_size
            torch.cuda.empty_cache()

            for call, ms, f, smp, same in results:
                med = ms[len(ms) // 2]
                row = dict(stream=name, cut=label, call=call, fragments=f, samples=smp, agrees_with_mp4_fragment=same,
                           kernel_ms_min=round(ms[0], 4), kernel_ms_median=round(med, 4), kernel_ms_max=round(ms[-1], 4), repeats=len(ms),
                           ns_per_sample=round(med * 1e6 / max(smp, 1), 2))
                box = ""
                if "one segment" in call:                      # the chain's cost: top-level boxes, a moof and an mdat a fragment
                    row["us_per_box"] = round(med * 1e3 / max(2 * f, 1), 3)
                    box = "%7.3f us a box" % row["us_per_box"]
                rows.append(row)
                print("%-44s %-22s %-80s %10.3f ms (min %10.3f, max %10.3f of %d)  %8d fragments %8d samples  %8.2f ns a sample  %-16s %s"
                      % (name, label, call, med, ms[0], ms[-1], len(ms), f, smp, row["ns_per_sample"], box,
                         "" if same is None else "agrees" if same else "DIFFERS"), flush=True)
        del stream, d_idx, d_au, d_nal_au
        torch.cuda.empty_cache()
    print(json.dumps({"mp4rd_time": rows, "source_digest": hbs.source_digest()}))


if __name__ == "__main__":
    main()
