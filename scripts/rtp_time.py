#!/usr/bin/env python3
"""Kernel time of hbs_rtp_pack (the library's HIP events around all of a call's launches, hbs_ctx_kernel_ms) on the bench stream
-- S(0x1234, n) of ~10 KiB NALs, 16 GiB by default -- and on a stream of ~1 KiB NALs (scripts/nal_sweep.py's shape, 2 GiB by
default), with max_payload 1188 and 8948 and both framings; access units of --au-nals NALs, a time per AU.  NALs whose type is
48 or above are filtered out first (hbs_filter_annexb with a d_keep mask), as the call's specification asks; the call then runs
on the filter's output and its index.  Next to it, in the same process and on the same stream, hbs_filter_annexb keep-all: the
plain copy of the same NALs.  Traffic = the NAL bytes read + the output bytes written; the index (32 B a NAL, read by each plan
pass), the AU numbers and times and the 40 B a NAL of scratch are not counted.  Fractions of the 8 TB/s peak.
    python scripts/rtp_time.py [--gib 16] [--small-gib 2] [--reps 5] [--au-nals 8]"""
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
        yield "S(0x1234, %d) ~10 KiB NALs" % n, g["stream"][: g["stream_bytes"]], n
        del g
        arena, total, idx, n, stream, sb = make_stream(torch, np, ctx, 1024, int(args.small_gib * 2**30))
        del arena, idx
        yield "random payload, ~1 KiB NALs", stream[:sb], n

    def timed(call):
        ctx.enable_timing(True)
        call()                                          # warm-up
        for _ in range(args.reps):
            call()
        ms = sorted(ctx.kernel_ms_back(b) for b in range(args.reps))
        ctx.enable_timing(False)
        return ms

    for name, raw, n_raw in shapes():
        ent, _, s = ctx.index_extract(raw, index_cap=n_raw + 16, want_rbsp=False)
        assert len(ent) == n_raw, (len(ent), n_raw)
        # what a receiver would read as AP / FU / PACI goes: the call refuses such NALs
        d_idx = torch.from_numpy(ent.view(np.uint8).copy()).to(dev)
        first = raw[torch.from_numpy(ent["start"].astype(np.int64)).to(dev)]
        long_enough = torch.from_numpy((ent["end"] - ent["start"] >= 2)).to(dev)
        keep = ((((first >> 1) & 63) < 48) & long_enough).to(torch.uint8)
        n = int(keep.sum().item())
        summ = torch.zeros(64, dtype=torch.uint8, device=dev)
        stream = torch.empty(raw.numel() + 16, dtype=torch.uint8, device=dev)
        index = torch.empty(n_raw * 32, dtype=torch.uint8, device=dev)
        ctx.filter_annexb_async(raw, raw.numel(), d_idx, n_raw, stream, index, summ, keep=keep)
        fs = ctx.read_summary(summ)
        assert int(fs["error"]) == 0 and int(fs["nal_count"]) == n, fs
        sb = int(fs["stream_bytes"])
        del raw, d_idx, first, keep, ent
        torch.cuda.empty_cache()
        stream, index = stream[:sb], index[: n * 32]
        lens = index.cpu().numpy().view(hbs.NAL_ENTRY)
        nal_bytes = int((lens["end"] - lens["start"]).sum())
        del lens

        n_aus = (n + args.au_nals - 1) // args.au_nals
        d_nal_au = torch.from_numpy((np.arange(n) // args.au_nals).astype(np.uint32).view(np.uint8).copy()).to(dev)
        d_pts = torch.from_numpy(((np.arange(n_aus, dtype=np.uint64) * np.uint64(3003)) & np.uint64((1 << 33) - 1)).view(np.uint8).copy()).to(dev)

        copy = torch.empty(sb + 16, dtype=torch.uint8, device=dev)
        copy_index = torch.empty(n * 32, dtype=torch.uint8, device=dev)
        rule = ctx.nal_filter()

        def keep_all():
            ctx.filter_annexb_async(stream, sb, index, n, copy, copy_index, summ, rule=rule)
        filter_ms = timed(keep_all)
        fs = ctx.read_summary(summ)
        assert int(fs["error"]) == 0 and int(fs["nal_count"]) == n, fs
        f_med = filter_ms[len(filter_ms) // 2]
        f_traffic = 2 * int(fs["stream_bytes"])
        print("%-34s %-44s %8.3f ms (min %8.3f)  %7.0f GB/s  %.3f of 8 TB/s (bytes read + bytes written)"
              % (name, "hbs_filter_annexb keep-all", f_med, filter_ms[0], f_traffic / f_med / 1e6, f_traffic / f_med / 1e6 / HBM_PEAK_GBS), flush=True)
        rows.append(dict(stream=name, call="hbs_filter_annexb keep-all", nals=n, kernel_ms_min=round(filter_ms[0], 4), kernel_ms_median=round(f_med, 4),
                         traffic_bytes=f_traffic, fraction_of_8tbs=round(f_traffic / f_med / 1e6 / HBM_PEAK_GBS, 3)))
        del copy, copy_index
        torch.cuda.empty_cache()

        for mp in (1188, 8948):
            for framing in (0, 2):
                prm = hbs.rtp_params(max_payload=mp, framing=framing, seq=65000, ts_base=12345, ssrc=0xCAFEF00D)
                a = (stream, sb, index, n, d_nal_au, n_aus, d_pts, prm)
                assert ctx.rtp_pack_async(*a, None, None, None, summ) == 0
                plan = ctx.read_summary(summ)
                assert int(plan["error"]) == 0 and int(plan["rbsp_bytes"]) == nal_bytes, plan
                out_bytes, packets = int(plan["stream_bytes"]), int(plan["nal_count"])
                out = torch.empty(out_bytes + 16, dtype=torch.uint8, device=dev)
                nal_off, nal_packet = (torch.empty((n + 1) * 8, dtype=torch.uint8, device=dev) for _ in range(2))

                def pack():
                    assert ctx.rtp_pack_async(*a, out, nal_off, nal_packet, summ, out_cap=out_bytes) == 0
                ms = timed(pack)
                sm = ctx.read_summary(summ)
                assert int(sm["error"]) == 0 and int(sm["stream_bytes"]) == out_bytes and int(sm["nal_count"]) == packets, sm
                # the first and the last packet, read as a receiver would
                off = nal_off.cpu().numpy().view(np.uint64)
                pk = nal_packet.cpu().numpy().view(np.uint64)
                stride = framing + 12 + mp
                head = hbs.rtp_packet(out[framing:min(stride, int(off[1]))].cpu().numpy())
                assert int(head["seq"]) == 65000 and int(head["timestamp"]) == 12345 and int(head["ssrc"]) == 0xCAFEF00D, head
                last_at = int(off[n - 1]) + int(pk[n] - pk[n - 1] - 1) * stride
                tail = hbs.rtp_packet(out[last_at + framing:out_bytes].cpu().numpy())
                assert int(tail["marker"]) == 1 and int(tail["seq"]) == (65000 + packets - 1) & 0xFFFF, tail
                med = ms[len(ms) // 2]
                traffic = nal_bytes + out_bytes
                row = dict(stream=name, call="hbs_rtp_pack", max_payload=mp, framing=framing, nals=n, fu_nals=int(sm["reserved"][2]), packets=packets,
                           nal_bytes=nal_bytes, out_bytes=out_bytes, kernel_ms_min=round(ms[0], 4), kernel_ms_median=round(med, 4), traffic_bytes=traffic,
                           gbs=round(traffic / med / 1e6, 1), fraction_of_8tbs=round(traffic / med / 1e6 / HBM_PEAK_GBS, 3),
                           time_over_filter=round(med / f_med, 3))
                rows.append(row)
                print("%-34s %-44s %8.3f ms (min %8.3f)  %7.0f GB/s  %.3f of 8 TB/s (bytes read + bytes written)  %.3f x the filter's time"
                      % (name, "hbs_rtp_pack max_payload %d framing %d" % (mp, framing), med, ms[0], row["gbs"], row["fraction_of_8tbs"],
                         row["time_over_filter"]), flush=True)
                del out, nal_off, nal_packet
                torch.cuda.empty_cache()
        del stream, index, d_nal_au, d_pts
        torch.cuda.empty_cache()
    print(json.dumps({"rtp_time": rows, "source_digest": hbs.source_digest()}))


if __name__ == "__main__":
    main()
