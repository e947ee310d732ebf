#!/usr/bin/env python3
"""Time of hbs_mp4_protect (HIP events around each call, same process), all tables written, on the fragments hbs_mp4_fragment
makes of the bench stream -- S(0x1234, n) of ~10 KiB NALs, 16 GiB by default, access units of --au-nals NALs, an IRAP every
32nd AU, HBS_MP4_CUT_AT_IRAP -- and of a stream of ~1 KiB NALs (scripts/nal_sweep.py's shape, one NAL an AU, 2 GiB by default)
two ways: cut at every 32nd AU, and max_samples 1 (a fragment a sample: the box-heavy worst case).  iv_size 8 and 0; the
subsample table is hbs_cenc_subsamples' with clear_lead 96 and no payload offsets.  Next to each row, in the same process and
timed the same way: hbs_mp4_fragment on the same data (the yardstick: it moves the same payload and writes a length field a NAL
and the trun arrays besides) and hbs_copy_device over the output's byte count.
    python scripts/mp4protect_time.py [--gib 16] [--small-gib 2] [--reps 5] [--au-nals 8]"""
import argparse
import ctypes as C
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
    ctx.lib.hbs_copy_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
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

    for name, stream, n, per, modes in shapes():
        sb = stream.numel()
        ent, _, s = ctx.index_extract(stream, index_cap=n + 16, want_rbsp=False)
        assert len(ent) == n, (len(ent), n)
        n_aus = (n + per - 1) // per
        au = np.zeros(n_aus, dtype=hbs.ACCESS_UNIT)
        au["flags"] = np.where(np.arange(n_aus) % 32 == 0, hbs.AU_IRAP, 0)
        d_idx, d_au, d_nal_au = up(ent), up(au), up((np.arange(n, dtype=np.int64) // per).astype(np.uint32))
        del ent
        summ = torch.zeros(64, dtype=torch.uint8, device=dev)
        # the subsample table: the same for every way of cutting
        first = torch.empty((n_aus + 1) * 8, dtype=torch.uint8, device=dev)
        b = (stream, sb, d_idx, n, d_nal_au, n_aus, hbs.cenc_plan_params(length_size=4, clear_lead=96), first)
        assert ctx.cenc_subsamples_async(*b, None, summ) == 0
        sp = ctx.read_summary(summ)
        assert int(sp["error"]) == 0, sp
        entries = int(sp["nal_count"])
        sub = torch.empty(max(entries, 2) * 8, dtype=torch.uint8, device=dev)
        assert ctx.cenc_subsamples_async(*b, sub, summ, sub_cap=entries) == 0
        assert int(ctx.read_summary(summ)["error"]) == 0
        iv = torch.zeros(n_aus * 16, dtype=torch.uint8, device=dev)
        iv.view(n_aus, 16)[:, :8] = torch.randint(0, 256, (n_aus, 8), dtype=torch.uint8, device=dev)

        for label, kw in modes:
            prm = hbs.mp4_params(length_size=4, track_id=1, sequence=1, sample_duration=3003, **kw)
            a = (stream, sb, d_idx, n, d_nal_au, d_au, n_aus, prm)
            assert ctx.mp4_fragment_async(*a, None, summ) == 0
            plan = ctx.read_summary(summ)
            assert int(plan["error"]) == 0, plan
            fbytes, frags = int(plan["stream_bytes"]), int(plan["nal_count"])
            fout = torch.empty(fbytes + 16, dtype=torch.uint8, device=dev)
            so, ss = (torch.empty(n_aus * 8, dtype=torch.uint8, device=dev) for _ in range(2))
            fr = torch.empty(frags * hbs.MP4_FRAG.itemsize, dtype=torch.uint8, device=dev)

            def fragment():
                assert ctx.mp4_fragment_async(*a, fout, summ, sample_off=so, sample_size=ss, frag=fr, frag_cap=frags, out_cap=fbytes) == 0
            f_ms = timed(fragment)
            assert int(ctx.read_summary(summ)["error"]) == 0
            f_med = f_ms[len(f_ms) // 2]
            for V in (8, 0):
                pp = hbs.mp4_protect_params(iv_size=V)
                p = (fout, fbytes, fr, frags, first, sub, iv if V else None, n_aus, pp)
                assert ctx.mp4_protect_async(*p, None, summ) == 0
                plan = ctx.read_summary(summ)
                assert int(plan["error"]) == 0, plan
                need = int(plan["stream_bytes"])
                assert need == fbytes + 53 * frags + (V + 3) * n_aus + 6 * entries and int(plan["rbsp_bytes"]) == entries
                out = torch.empty(need + 16, dtype=torch.uint8, device=dev)
                so2, ss2 = (torch.empty(n_aus * 8, dtype=torch.uint8, device=dev) for _ in range(2))
                fr2 = torch.empty(frags * hbs.MP4_FRAG.itemsize, dtype=torch.uint8, device=dev)

                def protect():
                    assert ctx.mp4_protect_async(*p, out, summ, sample_off=so2, sample_size=ss2, frag_out=fr2, out_cap=need) == 0
                ms = timed(protect)
                sm = ctx.read_summary(summ)
                assert int(sm["error"]) == 0 and int(sm["stream_bytes"]) == need, sm
                # spot check, reported and not asserted: the first fragment's boxes, and the last sample against the input's
                S0 = int(fr[: hbs.MP4_FRAG.itemsize].cpu().numpy().view(hbs.MP4_FRAG)[0]["samples"])
                head = out[:8].cpu().numpy().tobytes()
                o_in, o_out = (int(t[(n_aus - 1) * 8: n_aus * 8].cpu().numpy().view(np.uint64)[0]) for t in (so, so2))
                z = int(ss2[(n_aus - 1) * 8: n_aus * 8].cpu().numpy().view(np.uint64)[0])
                same = (head[4:] == b"moof" and out[88 + 16 * S0 + 4: 88 + 16 * S0 + 8].cpu().numpy().tobytes() == b"saiz" and o_out + z == need
                        and bool(torch.equal(out[o_out: o_out + z], fout[o_in: o_in + z])))
                dst = torch.empty(need + 16, dtype=torch.uint8, device=dev)
                c_ms = timed(lambda: ctx.lib.hbs_copy_device(ctx.h, C.c_void_p(dst.data_ptr()), C.c_void_p(out.data_ptr()), need))
                del dst
                med, c_med = ms[len(ms) // 2], c_ms[len(c_ms) // 2]
                row = dict(stream=name, cut=label, iv_size=V, nals=n, aus=n_aus, fragments=frags, entries=entries, in_bytes=fbytes, out_bytes=need,
                           last_sample_checks=same, protect_ms_median=round(med, 4), protect_ms_min=round(ms[0], 4),
                           fragment_ms_median=round(f_med, 4), fragment_ms_min=round(f_ms[0], 4), copy_ms_median=round(c_med, 4),
                           copy_ms_min=round(c_ms[0], 4), gbs_read_plus_written=round((fbytes + need) / med / 1e6, 1),
                           protect_over_fragment=round(med / f_med, 3), protect_over_copy=round(med / c_med, 3))
                rows.append(row)
                print("%-44s %-22s iv_size %2d  hbs_mp4_protect %8.3f ms (min %8.3f)  %6.2f GiB out  %8d fragments  %6.0f GB/s read + written;  "
                      "hbs_mp4_fragment %8.3f ms (min %8.3f): %.3f x;  hbs_copy_device of the output %8.3f ms (min %8.3f): %.3f x;  checks %s"
                      % (name, label, V, med, ms[0], need / 2**30, frags, row["gbs_read_plus_written"], f_med, f_ms[0], row["protect_over_fragment"],
                         c_med, c_ms[0], row["protect_over_copy"], same), flush=True)
                del out, so2, ss2, fr2
                torch.cuda.empty_cache()
            del fout, so, ss, fr
            torch.cuda.empty_cache()
        del stream, d_idx, d_au, d_nal_au, first, sub, iv
        torch.cuda.empty_cache()
    print(json.dumps({"mp4protect_time": rows, "source_digest": hbs.source_digest()}))


if __name__ == "__main__":
    main()
