#!/usr/bin/env python3
"""Time of hbs_cbcs_crypt on the samples hbs_mp4_fragment wrote (HIP events on the stream around each call, one process; median
and minimum of --reps calls after a warm-up), on the streams of scripts/cenc_time.py: the bench stream -- S(0x1234, n) of ~10 KiB
NALs, 16 GiB by default, cut into access units of --au-nals NALs -- and a stream of ~1 KiB NALs, one NAL an AU, 2 GiB by
default.  The subsample table is hbs_cenc_subsamples' with clear_lead 96 and no payload offsets.  Encrypt and decrypt, each at
1:9 and at 1:0, with the constant IV (iv_mode 1, no d_iv).  Next to them, in the same process and over the same bytes:
hbs_cenc_crypt, and hbs_copy_device as the yardstick -- what moving every byte once costs.  Reported: ms, the GB/s of enciphered
bytes, AES blocks/s, and the ratio to the copy's time.  Before the timing, one encrypt and one decrypt at each pattern must
restore the first MiB and the last.
    python scripts/cbcs_time.py [--gib 16] [--small-gib 2] [--reps 5] [--au-nals 8] [--out profiles/r24/cbcs_time.txt]"""
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
        assert ctx.cenc_subsamples_async(*b, sub, summ, sub_cap=entries) == 0
        assert int(ctx.read_summary(summ)["error"]) == 0
        del stream
        torch.cuda.empty_cache()

        key, iv0 = bytes(range(16)), bytes(range(16, 32))
        head, last_at = out[: 1 << 20].clone(), max(need - (1 << 20), 0)
        last = out[last_at:need].clone()
        row = dict(stream=name, nals=n, aus=n_aus, entries=entries, fragment_bytes=need, protected_bytes=protected)
        parts = []
        for c, k in ((1, 9), (1, 0)):
            prms = [hbs.cbcs_params(key, iv0=iv0, flags=f, crypt_byte_block=c, skip_byte_block=k) for f in (0, hbs.CBCS_DECRYPT)]
            calls = [lambda p=p: ctx.cbcs_crypt_async(out, need, so, ss, n_aus, first, sub, None, p, summ) for p in prms]
            # there and back once: the fragments are restored
            assert calls[0]() == 0
            se = ctx.read_summary(summ)
            assert int(se["error"]) == 0 and int(se["nal_count"]) == entries, se
            done = int(se["rbsp_bytes"])
            changed = not bool(torch.equal(out[: 1 << 20], head))
            assert calls[1]() == 0
            sd = ctx.read_summary(summ)
            assert int(sd["error"]) == 0 and int(sd["rbsp_bytes"]) == done, sd
            restored = bool(torch.equal(out[: 1 << 20], head)) and bool(torch.equal(out[last_at:need], last))
            assert changed and restored, (changed, restored)
            for what, call in zip(("encrypt", "decrypt"), calls):
                ms = timed(call)
                med = ms[len(ms) // 2]
                tag = "cbcs_%s_%d_%d" % (what, c, k)
                row[tag + "_ms_median"], row[tag + "_ms_min"] = round(med, 4), round(ms[0], 4)
                row[tag + "_gbs"], row[tag + "_aes_blocks_per_s"] = round(done / med / 1e6, 1), round(done / 16 / med * 1e3)
                parts.append("hbs_cbcs_crypt %s %d:%d %9.3f ms (min %9.3f) = %7.1f enciphered GB/s, %.3e AES blocks/s" %
                             (what, c, k, med, ms[0], done / med / 1e6, done / 16 / med * 1e3))
            row["cbcs_%d_%d_enciphered_bytes" % (c, k)] = done
        # (the timed calls leave other bytes than the fragments: the work of the calls below does not depend on them)

        kprm = hbs.cenc_params(bytes(range(16)), iv0=bytes(8))
        c_ms = timed(lambda: ctx.cenc_crypt_async(out, need, so, ss, n_aus, first, sub, None, kprm, summ))
        sc = ctx.read_summary(summ)
        assert int(sc["error"]) == 0 and int(sc["rbsp_bytes"]) == protected, sc

        # the yardstick: the same bytes copied once
        dst = torch.empty(need + 16, dtype=torch.uint8, device=dev)
        ctx._bind_stream()
        y_ms = timed(lambda: ctx.lib.hbs_copy_device(ctx.h, C.c_void_p(dst.data_ptr()), C.c_void_p(out.data_ptr()), need))
        del dst

        c_med, y_med = c_ms[len(c_ms) // 2], y_ms[len(y_ms) // 2]
        row.update(cenc_crypt_ms_median=round(c_med, 4), cenc_crypt_ms_min=round(c_ms[0], 4), copy_ms_median=round(y_med, 4), copy_ms_min=round(y_ms[0], 4),
                   copy_gbs_read_plus_written=round(2 * need / y_med / 1e6, 1))
        for tag in [t for t in row if t.startswith("cbcs_") and t.endswith("_ms_median")]:
            row[tag[: -len("_ms_median")] + "_over_copy"] = round(row[tag] / y_med, 3)
        rows.append(row)
        line = ("%-44s %d samples, %d entries, %.2f GiB of fragments, %.2f GiB protected: %s; hbs_cenc_crypt %9.3f ms (min %9.3f); "
                "hbs_copy_device of the fragments %8.3f ms (min %8.3f, %6.0f GB/s read + written)" %
                (name, n_aus, entries, need / 2**30, protected / 2**30, "; ".join(parts), c_med, c_ms[0], y_med, y_ms[0], row["copy_gbs_read_plus_written"]))
        print(line, flush=True)
        lines.append(line)
        del out, so, ss, fr, first, sub, d_idx, d_au, d_nal_au
        torch.cuda.empty_cache()
    tail = json.dumps({"cbcs_time": rows, "source_digest": hbs.source_digest()})
    print(tail)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines + [tail]) + "\n")


if __name__ == "__main__":
    main()
