#!/usr/bin/env python3
"""Time of hbs_cenc_crypt on the samples hbs_mp4_fragment wrote (HIP events on the stream around each call, one process; median
and minimum of --reps calls after a warm-up), on the bench stream -- S(0x1234, n) of ~10 KiB NALs, 16 GiB by default, cut into
access units of --au-nals NALs -- and on a stream of ~1 KiB NALs (scripts/nal_sweep.py's shape, one NAL an AU, 2 GiB by default).
The subsample table is hbs_cenc_subsamples' with clear_lead 96 and no payload offsets: every NAL whose first byte says VCL (the
payload is random: about half of them) is protected behind its first 96 bytes.  Sequential IVs (iv_mode 1), no d_iv.  Next to
it, in the same process: hbs_cenc_subsamples itself, and hbs_copy_device over the same fragment bytes as the yardstick -- what
moving every byte once costs.  Reported: ms, protected GB/s, AES blocks/s, and the ratio to the copy's time.
    python scripts/cenc_time.py [--gib 16] [--small-gib 2] [--reps 5] [--au-nals 8] [--out profiles/r23/cenc_time.txt]"""
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import hevcbitstream_amd as hbs
    from scripts.nal_sweep import make_stream

    ctx = hbs.Context(0)
    dev = torch.device("cuda", 0)
    ctx.lib.hbs_copy_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
    rows, lines = [], []

    def shapes():
        n = int(round(104_858 * args.gib))
        g = ctx.synth_stream(0x1234, n, 0)
        yield "S(0x1234, %d) ~10 KiB NALs, AUs of %d NALs" % (n, args.au_nals), g["stream"][: g["stream_bytes"]], n, args.au_nals
        del g
        arena, total, idx, n, stream, sb = make_stream(torch, np, ctx, 1024, int(args.small_gib * 2**30))
        del arena, idx
        yield "random payload, AUs of one ~1 KiB NAL", stream[:sb], n, 1

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

    for name, stream, n, per in shapes():
        sb = stream.numel()
        ent, _, s = ctx.index_extract(stream, index_cap=n + 16, want_rbsp=False)
        assert len(ent) == n, (len(ent), n)
        n_aus = (n + per - 1) // per
        au = np.zeros(n_aus, dtype=hbs.ACCESS_UNIT)
        au["flags"] = np.where(np.arange(n_aus) % 32 == 0, hbs.AU_IRAP, 0)
        d_idx, d_au, d_nal_au = up(ent), up(au), up((np.arange(n, dtype=np.int64) // per).astype(np.uint32))
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

        # the subsample table
        cprm = hbs.cenc_plan_params(length_size=4, clear_lead=96)
        first = torch.empty((n_aus + 1) * 8, dtype=torch.uint8, device=dev)
        b = (stream, sb, d_idx, n, d_nal_au, n_aus, cprm, first)
        assert ctx.cenc_subsamples_async(*b, None, summ) == 0
        sp = ctx.read_summary(summ)
        assert int(sp["error"]) == 0, sp
        entries, protected = int(sp["nal_count"]), int(sp["rbsp_bytes"])
        sub = torch.empty(max(entries, 2) * 8, dtype=torch.uint8, device=dev)
        p_ms = timed(lambda: ctx.cenc_subsamples_async(*b, sub, summ, sub_cap=entries))
        assert int(ctx.read_summary(summ)["error"]) == 0
        del stream
        torch.cuda.empty_cache()

        # the cipher, in place: an even number of calls leaves the fragments as they were
        kprm = hbs.cenc_params(bytes(range(16)), iv0=bytes(8))
        before = out[: 1 << 20].clone()
        c_ms = timed(lambda: ctx.cenc_crypt_async(out, need, so, ss, n_aus, first, sub, None, kprm, summ))
        sc = ctx.read_summary(summ)
        assert int(sc["error"]) == 0 and int(sc["rbsp_bytes"]) == protected and int(sc["nal_count"]) == entries, sc
        changed = not bool(torch.equal(out[: 1 << 20], before)) if (args.reps + 1) % 2 else bool(torch.equal(out[: 1 << 20], before))

        # the yardstick: the same bytes copied once
        dst = torch.empty(need + 16, dtype=torch.uint8, device=dev)
        ctx._bind_stream()
        y_ms = timed(lambda: ctx.lib.hbs_copy_device(ctx.h, C.c_void_p(dst.data_ptr()), C.c_void_p(out.data_ptr()), need))
        del dst

        c_med, y_med, p_med = c_ms[len(c_ms) // 2], y_ms[len(y_ms) // 2], p_ms[len(p_ms) // 2]
        blocks = (protected + 15) // 16
        row = dict(stream=name, nals=n, aus=n_aus, entries=entries, fragment_bytes=need, protected_bytes=protected,
                   crypt_ms_median=round(c_med, 4), crypt_ms_min=round(c_ms[0], 4), protected_gbs=round(protected / c_med / 1e6, 1),
                   aes_blocks_per_s=round(blocks / c_med * 1e3), subsamples_ms_median=round(p_med, 4), subsamples_ms_min=round(p_ms[0], 4),
                   copy_ms_median=round(y_med, 4), copy_ms_min=round(y_ms[0], 4), copy_gbs_read_plus_written=round(2 * need / y_med / 1e6, 1),
                   crypt_over_copy=round(c_med / y_med, 3), first_mib_as_expected=changed)
        rows.append(row)
        line = ("%-44s %d samples, %d entries, %.2f GiB of fragments, %.2f GiB protected: hbs_cenc_crypt %9.3f ms (min %9.3f) = %7.1f protected GB/s, "
                "%.3e AES blocks/s; hbs_cenc_subsamples %8.3f ms (min %8.3f); hbs_copy_device of the fragments %8.3f ms (min %8.3f, %6.0f GB/s read + written); "
                "crypt / copy = %.2f" % (name, n_aus, entries, need / 2**30, protected / 2**30, c_med, c_ms[0], row["protected_gbs"], blocks / c_med * 1e3,
                                        p_med, p_ms[0], y_med, y_ms[0], row["copy_gbs_read_plus_written"], c_med / y_med))
        print(line, flush=True)
        lines.append(line)
        del out, so, ss, fr, first, sub, d_idx, d_au, d_nal_au
        torch.cuda.empty_cache()
    tail = json.dumps({"cenc_time": rows, "source_digest": hbs.source_digest()})
    print(tail)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines + [tail]) + "\n")


if __name__ == "__main__":
    main()
