#!/usr/bin/env python3
"""Kernel time of hbs_mp4_stbl_samples (the library's HIP events around all of a call's launches, hbs_ctx_kernel_ms), all five
tables written, for the two README shapes: the bench stream S(0x1234, n) of ~10 KiB NALs, 16 GiB by default, AUs of --au-nals
NALs; and ~1 KiB NALs, one an AU, 2 GiB by default.  The samples are those hbs_mp4_fragment writes (cut at every 32nd AU); the
progressive file's tables describe them where they lie, in chunks of 32: a stsz of N sizes, a co64 of a chunk a fragment, a
stsc of one entry, a stts of one entry, a stss of every 32nd sample -- and once more with a ctts of one entry a sample.  Next
to it, in the same process and on the same samples: hbs_mp4_samples on the fragments of 32 (the fragment table as segments),
and hbs_lenpref_to_annexb on the table this call wrote.  And one plan-only row.
    python scripts/mp4stbl_time.py [--gib 16] [--small-gib 2] [--reps 5] [--au-nals 8]"""
import argparse
import json
import os
import struct
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

    def be(x, width):
        return np.asarray(x).astype(">u%d" % width).tobytes()

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
        fr = torch.empty(frags * hbs.MP4_FRAG.itemsize, dtype=torch.uint8, device=dev)
        assert ctx.mp4_fragment_async(*a, out, summ, sample_off=so, sample_size=ss, frag=fr, frag_cap=frags, out_cap=need) == 0
        assert int(ctx.read_summary(summ)["error"]) == 0
        h_off, h_size = so.cpu().numpy().view(np.uint64), ss.cpu().numpy().view(np.uint64)
        chunks = (n_aus + 31) // 32
        assert chunks == frags

        # the tables of the progressive file that holds these samples where they lie
        def tables(ctts):
            pay = dict(stsz=struct.pack(">III", 0, 0, n_aus) + be(h_size, 4), stco=struct.pack(">II", 0, chunks) + be(h_off[::32], 8),
                       stsc=struct.pack(">IIIII", 0, 1, 1, 32, 1), stts=struct.pack(">IIII", 0, 1, n_aus, 3003),
                       stss=struct.pack(">II", 0, chunks) + be(np.arange(1, n_aus + 1, 32), 4))
            if ctts:
                pairs = np.empty((n_aus, 2), dtype=">u4")
                pairs[:, 0], pairs[:, 1] = 1, 3003 * (np.arange(n_aus) % 3)
                pay["ctts"] = struct.pack(">II", 0, n_aus) + pairs.tobytes()
            rec = np.zeros(1, dtype=hbs.MP4_STBL)
            buf = bytearray()
            for k, v in pay.items():
                buf += bytes(-len(buf) % 16)
                rec[k][0] = (len(buf), len(v))
                buf += v
            rec["flags"], rec["file_bytes"] = hbs.MP4_STBL_CO64, need
            return up(np.frombuffer(bytes(buf), dtype=np.uint8)), len(buf), rec

        t_off, t_size, t_dts, t_pts = (torch.empty(n_aus * 8, dtype=torch.uint8, device=dev) for _ in range(4))
        t_fl = torch.empty(n_aus * 4, dtype=torch.uint8, device=dev)
        outs = dict(sample_off=t_off, sample_size=t_size, dts=t_dts, pts=t_pts, sample_flags=t_fl)
        results = []
        for label, ctts in (("chunks of 32, stts of one entry", False), ("the same with a ctts of one entry a sample", True)):
            d_tbl, tb, rec = tables(ctts)

            def stbl():
                assert ctx.mp4_stbl_samples_async(d_tbl, tb, rec, summ, sample_cap=n_aus, **outs) == 0
            ms = timed(stbl, args.reps)
            sm = ctx.read_summary(summ)
            same = (int(sm["error"]) == 0 and int(sm["nal_count"]) == n_aus and int(sm["nal_found"]) == chunks
                    and bool(torch.equal(t_off, so)) and bool(torch.equal(t_size, ss)))
            results.append(("hbs_mp4_stbl_samples, " + label, ms, same))
            if not ctts:
                def plan_only():
                    assert ctx.mp4_stbl_samples_async(d_tbl, tb, rec, summ) == 0
                ms = timed(plan_only, args.reps)
                sm = ctx.read_summary(summ)
                same = int(sm["error"]) == 0 and int(sm["nal_count"]) == n_aus and int(sm["rbsp_bytes"]) == int(h_size.sum())
                results.append(("hbs_mp4_stbl_samples, plan only, chunks of 32", ms, same))
            del d_tbl

        # the same samples as fragments of 32
        rp = hbs.mp4_read_params(track_id=1)
        f_off, f_size = (torch.empty(n_aus * 8, dtype=torch.uint8, device=dev) for _ in range(2))
        t_fr = torch.empty(frags * hbs.MP4_FRAG.itemsize, dtype=torch.uint8, device=dev)

        def by_table():
            assert ctx.mp4_samples_async(out, need, rp, summ, seg=fr, seg_stride=hbs.MP4_FRAG.itemsize, n_segs=frags, moof_cap=frags,
                                         sample_cap=n_aus, sample_off=f_off, sample_size=f_size, dts=t_dts, pts=t_pts, sample_flags=t_fl, frag=t_fr) == 0
        ms = timed(by_table, args.reps)
        sm = ctx.read_summary(summ)
        same = int(sm["error"]) == 0 and bool(torch.equal(f_off, t_off)) and bool(torch.equal(f_size, t_size))
        results.append(("hbs_mp4_samples, the samples as fragments of 32 (fragment table as segments)", ms, same))
        del f_off, f_size, t_fr, t_dts, t_pts, t_fl

        # the copy the table feeds
        assert ctx.lenpref_to_annexb_async(out, need, t_off, t_size, n_aus, None, None, summ, length_size=4, startcode_bytes=4, nal_cap=1 << 62) == 0
        lp = ctx.read_summary(summ)
        assert int(lp["error"]) == 0, lp
        back_bytes, recs = int(lp["stream_bytes"]), int(lp["nal_count"])
        back = torch.empty(back_bytes + 16, dtype=torch.uint8, device=dev)

        def annexb():
            assert ctx.lenpref_to_annexb_async(out, need, t_off, t_size, n_aus, back, None, summ, length_size=4, startcode_bytes=4,
                                               nal_cap=recs, out_cap=back_bytes) == 0
        results.append(("hbs_lenpref_to_annexb on that table", timed(annexb, args.reps), int(ctx.read_summary(summ)["error"]) == 0))
        del back, out, so, ss, fr, t_off, t_size
        torch.cuda.empty_cache()

        for call, ms, same in results:
            med = ms[len(ms) // 2]
            row = dict(stream=name, call=call, chunks=chunks, samples=n_aus, agrees_with_mp4_fragment=same, kernel_ms_min=round(ms[0], 4),
                       kernel_ms_median=round(med, 4), kernel_ms_max=round(ms[-1], 4), repeats=len(ms), ns_per_sample=round(med * 1e6 / max(n_aus, 1), 2))
            rows.append(row)
            print("%-44s %-82s %10.3f ms (min %10.3f, max %10.3f of %d)  %8d chunks %8d samples  %8.2f ns a sample  %s"
                  % (name, call, med, ms[0], ms[-1], len(ms), chunks, n_aus, row["ns_per_sample"], "agrees" if same else "DIFFERS"), flush=True)
        del stream, d_idx, d_au, d_nal_au
        torch.cuda.empty_cache()
    print(json.dumps({"mp4stbl_time": rows, "source_digest": hbs.source_digest()}))


if __name__ == "__main__":
    main()
