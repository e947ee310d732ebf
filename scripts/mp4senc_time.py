#!/usr/bin/env python3
"""Time of hbs_mp4_senc_samples (HIP events around each call, same process), all tables written, on the protected fragments
hbs_mp4_fragment + hbs_mp4_protect (iv_size 8) make of the bench stream -- S(0x1234, n) of ~10 KiB NALs, 16 GiB by default, access
units of --au-nals NALs, an IRAP every 32nd AU, HBS_MP4_CUT_AT_IRAP -- and of a stream of ~1 KiB NALs (scripts/nal_sweep.py's
shape, one NAL an AU, 2 GiB by default) two ways: cut at every 32nd AU, and max_samples 1.  Next to each row, in the same process
and timed the same way: hbs_mp4_samples with all six tables on the same protected bytes (the yardstick: it opens the same moofs
and reads a comparable number of bytes a sample) and hbs_cenc_crypt decrypting them with the tables read back.
hbs_mp4_samples is given the whole buffer as one segment, so in the rows of many fragments its time is that of the one lane that
walks the chain of top-level boxes: only the one-fragment rows compare like with like.
One more row a stream: all samples in ONE fragment (a fragment's mdat has a 32-bit size, so of the first stream only its first
--one-gib GiB), read with its saiz (a lane a sample) and again with the saiz renamed 'free' (one lane walks the whole senc): the
serial walk's cost, for the record.
    python scripts/mp4senc_time.py [--gib 16] [--small-gib 2] [--one-gib 3] [--reps 5] [--au-nals 8]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=16.0)
    ap.add_argument("--small-gib", type=float, default=2.0)
    ap.add_argument("--one-gib", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--au-nals", type=int, default=8)
    args = ap.parse_args()
    import numpy as np
    import torch
    import hevcbitstream_amd as hbs
    from scripts.nal_sweep import make_stream

    ctx = hbs.Context(0)
    dev = torch.device("cuda", 0)
    FRAG = hbs.MP4_FRAG.itemsize
    rows = []

    def shapes():
        n = int(round(104_858 * args.gib))
        g = ctx.synth_stream(0x1234, n, 0)
        yield ("S(0x1234, %d) ~10 KiB NALs, AUs of %d NALs" % (n, args.au_nals), g["stream"][: g["stream_bytes"]], n, args.au_nals,
               (("cut at every 32nd AU", dict(flags=hbs.MP4_CUT_AT_IRAP), 1.0),
                ("one fragment (first %.1f GiB)" % args.one_gib, dict(flags=0, max_samples=0), min(1.0, args.one_gib / args.gib))))
        del g
        arena, total, idx, n, stream, sb = make_stream(torch, np, ctx, 1024, int(args.small_gib * 2**30))
        del arena, idx
        yield ("random payload, AUs of one ~1 KiB NAL", stream[:sb], n, 1,
               (("cut at every 32nd AU", dict(flags=hbs.MP4_CUT_AT_IRAP), 1.0), ("max_samples 1", dict(max_samples=1), 1.0),
                ("one fragment", dict(flags=0, max_samples=0), 1.0)))

    def timed(call):
        call()                                          # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return sorted(ms)

    def up(x):
        return torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)

    def empty(nbytes):
        return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)

    for name, stream, n_all, per, modes in shapes():
        ent_all, _, s = ctx.index_extract(stream, index_cap=n_all + 16, want_rbsp=False)
        assert len(ent_all) == n_all, (len(ent_all), n_all)
        for label, kw, part in modes:
            n = max(per, int(n_all * part) // per * per)
            ent = ent_all[:n]
            sb = int(ent["end"][-1]) if "end" in ent.dtype.names else stream.numel()
            n_aus = (n + per - 1) // per
            au = np.zeros(n_aus, dtype=hbs.ACCESS_UNIT)
            au["flags"] = np.where(np.arange(n_aus) % 32 == 0, hbs.AU_IRAP, 0)
            d_idx, d_au, d_nal_au = up(ent), up(au), up((np.arange(n, dtype=np.int64) // per).astype(np.uint32))
            summ = torch.zeros(64, dtype=torch.uint8, device=dev)
            first0 = empty((n_aus + 1) * 8)
            b = (stream, sb, d_idx, n, d_nal_au, n_aus, hbs.cenc_plan_params(length_size=4, clear_lead=96), first0)
            assert ctx.cenc_subsamples_async(*b, None, summ) == 0
            sp = ctx.read_summary(summ)
            assert int(sp["error"]) == 0, sp
            entries = int(sp["nal_count"])
            sub0 = empty(entries * 8)
            assert ctx.cenc_subsamples_async(*b, sub0, summ, sub_cap=entries) == 0
            assert int(ctx.read_summary(summ)["error"]) == 0
            iv0 = torch.zeros(n_aus * 16, dtype=torch.uint8, device=dev)
            iv0.view(n_aus, 16)[:, :8] = torch.randint(0, 256, (n_aus, 8), dtype=torch.uint8, device=dev)
            # the protected fragments
            prm = hbs.mp4_params(length_size=4, track_id=1, sequence=1, sample_duration=3003, **kw)
            a = (stream, sb, d_idx, n, d_nal_au, d_au, n_aus, prm)
            assert ctx.mp4_fragment_async(*a, None, summ) == 0
            plan = ctx.read_summary(summ)
            assert int(plan["error"]) == 0, plan
            fbytes, frags = int(plan["stream_bytes"]), int(plan["nal_count"])
            fout, fr = empty(fbytes), empty(frags * FRAG)
            assert ctx.mp4_fragment_async(*a, fout, summ, frag=fr, frag_cap=frags, out_cap=fbytes) == 0
            assert int(ctx.read_summary(summ)["error"]) == 0
            p = (fout, fbytes, fr, frags, first0, sub0, iv0, n_aus, hbs.mp4_protect_params(iv_size=8))
            assert ctx.mp4_protect_async(*p, None, summ) == 0
            need = int(ctx.read_summary(summ)["stream_bytes"])
            out = empty(need)
            assert ctx.mp4_protect_async(*p, out, summ, out_cap=need) == 0
            assert int(ctx.read_summary(summ)["error"]) == 0
            del fout, fr, d_idx, d_au, d_nal_au
            torch.cuda.empty_cache()
            # the yardstick: hbs_mp4_samples, all six tables
            so, ss, dt, pt = (empty(n_aus * 8) for _ in range(4))
            fl, fr2 = empty(n_aus * 4), empty(frags * FRAG)
            rp = hbs.mp4_read_params()

            def samples():
                assert ctx.mp4_samples_async(out, need, rp, summ, moof_cap=frags, sample_cap=n_aus, sample_off=so, sample_size=ss, dts=dt, pts=pt,
                                             sample_flags=fl, frag=fr2) == 0
            r_ms = timed(samples)
            sm = ctx.read_summary(summ)
            assert int(sm["error"]) == 0 and int(sm["nal_count"]) == n_aus and int(sm["nal_found"]) == frags, sm
            # the call: as written, and (one fragment) with the saiz renamed
            first, sub, iv = empty((n_aus + 1) * 8), empty(entries * 8), empty(n_aus * 16)
            sp_ = hbs.mp4_senc_params(iv_size=8)
            variants = [("as written", None)]
            if frags == 1:
                variants.append(("saiz renamed 'free'", 88 + 16 * n_aus + 4))
            for how, at in variants:
                if at is not None:
                    assert out[at:at + 4].cpu().numpy().tobytes() == b"saiz"
                    out[at:at + 4] = torch.from_numpy(np.frombuffer(b"free", dtype=np.uint8).copy()).to(dev)

                def senc():
                    assert ctx.mp4_senc_samples_async(out, need, fr2, frags, ss, n_aus, sp_, first, sub, iv, summ, sub_cap=entries) == 0
                ms = timed(senc)
                sm = ctx.read_summary(summ)
                assert int(sm["error"]) == 0 and int(sm["nal_count"]) == entries and int(sm["reserved"][2]) == frags, sm
                same = bool(torch.equal(first[: (n_aus + 1) * 8], first0[: (n_aus + 1) * 8]) and torch.equal(sub[: entries * 8], sub0[: entries * 8])
                            and torch.equal(iv[: n_aus * 16], iv0))
                kp = hbs.cenc_params(bytes(range(16)))
                c_ms = timed(lambda: ctx.cenc_crypt_async(out, need, so, ss, n_aus, first, sub, iv, kp, summ))
                assert int(ctx.read_summary(summ)["error"]) == 0
                med, r_med, c_med = ms[len(ms) // 2], r_ms[len(r_ms) // 2], c_ms[len(c_ms) // 2]
                row = dict(stream=name, cut=label, senc=how, nals=n, samples=n_aus, fragments=frags, entries=entries, in_bytes=need,
                           tables_equal_the_writers=same, senc_ms_median=round(med, 4), senc_ms_min=round(ms[0], 4), senc_ms_max=round(ms[-1], 4),
                           samples_ms_median=round(r_med, 4), samples_ms_min=round(r_ms[0], 4), samples_ms_max=round(r_ms[-1], 4),
                           crypt_ms_median=round(c_med, 4), senc_over_samples=round(med / r_med, 3), ns_per_sample=round(med * 1e6 / n_aus, 2))
                rows.append(row)
                print("%-44s %-30s %-20s hbs_mp4_senc_samples %8.3f ms (min %8.3f max %8.3f)  %8d samples %8d fragments %9d entries  %7.2f ns a sample;  "
                      "hbs_mp4_samples %8.3f ms (min %8.3f max %8.3f): %.3f x;  hbs_cenc_crypt %9.3f ms;  tables equal %s"
                      % (name, label, how, med, ms[0], ms[-1], n_aus, frags, entries, row["ns_per_sample"], r_med, r_ms[0], r_ms[-1],
                         row["senc_over_samples"], c_med, same), flush=True)
            del out, so, ss, dt, pt, fl, fr2, first, sub, iv, first0, sub0, iv0
            torch.cuda.empty_cache()
        del stream, ent_all
        torch.cuda.empty_cache()
    print(json.dumps({"mp4senc_time": rows, "source_digest": hbs.source_digest()}))


if __name__ == "__main__":
    main()
