#!/usr/bin/env python3
"""Kernel time of hbs_rtp_pack with and without HBS_RTP_AGGREGATE (the library's HIP events around all of a call's launches,
hbs_ctx_kernel_ms), next to hbs_filter_annexb keep-all -- the plain copy of the same NALs -- in the same process and on the same
stream: ~1 KiB NALs (scripts/nal_sweep.py's shape, 2 GiB by default) at max_payload 1188 and 8948, ~128-byte NALs (2 GiB) at
1188, and the bench stream S(0x1234, n) of ~10 KiB NALs (16 GiB) at 1188, where every NAL is sent as fragmentation units, no
aggregation packet can form and the flag's row shows what it costs when it does nothing.  Framing 0, access units of --au-nals
NALs, a time per AU.  NALs whose type is 48 or above are filtered out first, as in scripts/rtp_time.py.  Traffic = the NAL bytes
read + the output bytes written; the index, the AU numbers and times and the scratch are not counted.  Fractions of the 8 TB/s
peak.  A library that refuses the flag (HBS_LIB=... of an older build, for timing the flag-less call against it in one session)
gets the flag-less rows only.
    python scripts/rtpap_time.py [--gib 16] [--small-gib 2] [--reps 5] [--au-nals 8]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HBM_PEAK_GBS = 8000.0
AGGREGATE = 4


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
        for size, mps in ((1024, (1188, 8948)), (128, (1188,))):
            arena, total, idx, n, stream, sb = make_stream(torch, np, ctx, size, int(args.small_gib * 2**30))
            del arena, idx
            yield "random payload, ~%s NALs" % ("1 KiB" if size == 1024 else "%d-byte" % size), stream[:sb], n, mps
            del stream
            torch.cuda.empty_cache()
        if args.gib > 0:
            n = int(round(104_858 * args.gib))
            g = ctx.synth_stream(0x1234, n, 0)
            yield "S(0x1234, %d) ~10 KiB NALs" % n, g["stream"][: g["stream_bytes"]], n, (1188,)

    def timed(call):
        ctx.enable_timing(True)
        call()                                          # warm-up
        for _ in range(args.reps):
            call()
        ms = sorted(ctx.kernel_ms_back(b) for b in range(args.reps))
        ctx.enable_timing(False)
        return ms

    for name, raw, n_raw, mps in shapes():
        ent, _, s = ctx.index_extract(raw, index_cap=n_raw + 16, want_rbsp=False)
        assert len(ent) == n_raw, (len(ent), n_raw)
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
        del raw, d_idx, first, keep, ent, long_enough
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
        print("%-30s %-40s %8.3f ms (min %8.3f)  %7.0f GB/s  %.3f of 8 TB/s (bytes read + bytes written)"
              % (name, "hbs_filter_annexb keep-all", f_med, filter_ms[0], f_traffic / f_med / 1e6, f_traffic / f_med / 1e6 / HBM_PEAK_GBS), flush=True)
        rows.append(dict(stream=name, call="hbs_filter_annexb keep-all", nals=n, kernel_ms_min=round(filter_ms[0], 4), kernel_ms_median=round(f_med, 4),
                         traffic_bytes=f_traffic, fraction_of_8tbs=round(f_traffic / f_med / 1e6 / HBM_PEAK_GBS, 3)))
        del copy, copy_index
        torch.cuda.empty_cache()

        for mp in mps:
            plain_out = None
            for flags in (0, AGGREGATE):
                prm = hbs.rtp_params(max_payload=mp, framing=0, flags=flags, seq=65000, ts_base=12345, ssrc=0xCAFEF00D)
                a = (stream, sb, index, n, d_nal_au, n_aus, d_pts, prm)
                if ctx.rtp_pack_async(*a, None, None, None, summ) != 0:
                    assert flags, "the flag-less call was refused"
                    print("%-30s %-40s refused by this library" % (name, "hbs_rtp_pack max_payload %d AGGREGATE" % mp), flush=True)
                    continue
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
                # the first packet, read as a receiver would; the tables' last entries
                head = hbs.rtp_packet(out[:min(12 + mp, out_bytes)].cpu().numpy())
                assert int(head["seq"]) == 65000 and int(head["timestamp"]) == 12345 and int(head["ssrc"]) == 0xCAFEF00D, head
                assert int(nal_off[n * 8:].cpu().numpy().view(np.uint64)[0]) == out_bytes
                assert int(nal_packet[n * 8:].cpu().numpy().view(np.uint64)[0]) == packets
                if flags:
                    assert plain_out is not None and out_bytes <= plain_out
                else:
                    plain_out = out_bytes
                med = ms[len(ms) // 2]
                traffic = nal_bytes + out_bytes
                label = "hbs_rtp_pack max_payload %d%s" % (mp, " AGGREGATE" if flags else "")
                row = dict(stream=name, call=label, max_payload=mp, flags=flags, nals=n, fu_nals=int(sm["reserved"][2]) & 0xFFFFFFFF,
                           aps=int(sm["reserved"][2]) >> 32, packets=packets, nal_bytes=nal_bytes, out_bytes=out_bytes,
                           kernel_ms_min=round(ms[0], 4), kernel_ms_median=round(med, 4), kernel_ms_all=[round(x, 4) for x in ms],
                           traffic_bytes=traffic, gbs=round(traffic / med / 1e6, 1), fraction_of_8tbs=round(traffic / med / 1e6 / HBM_PEAK_GBS, 3),
                           time_over_filter=round(med / f_med, 3))
                rows.append(row)
                print("%-30s %-40s %8.3f ms (min %8.3f)  %7.0f GB/s  %.3f of 8 TB/s  %.3f x the filter's time  %d packets (%d APs, %d FU NALs), %d output bytes"
                      % (name, label, med, ms[0], row["gbs"], row["fraction_of_8tbs"], row["time_over_filter"], packets, row["aps"], row["fu_nals"],
                         out_bytes), flush=True)
                del out, nal_off, nal_packet
                torch.cuda.empty_cache()
        del stream, index, d_nal_au, d_pts
        torch.cuda.empty_cache()
    print(json.dumps({"rtpap_time": rows, "source_digest": hbs.source_digest(), "library": os.environ.get("HBS_LIB", "")}))


if __name__ == "__main__":
    main()
