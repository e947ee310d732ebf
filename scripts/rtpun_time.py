#!/usr/bin/env python3
"""Kernel time of hbs_rtp_unpack (the library's HIP events around all of a call's launches, hbs_ctx_kernel_ms) on the output of
hbs_rtp_pack: the bench stream -- S(0x1234, n) of ~10 KiB NALs, 16 GiB by default -- packed with max_payload 1188 and 8948, and
a stream of ~1 KiB NALs (scripts/nal_sweep.py's shape, 2 GiB by default) packed with max_payload 1188; packets back to back
(framing 0), access units of --au-nals NALs, a time per AU.  As in scripts/rtp_time.py, NALs whose type is 48 or above are
filtered out before they are packed.  Next to it, in the same process: hbs_rtp_pack on the same data, and hbs_filter_annexb
keep-all on the unpacked stream with the index the call wrote (the plain copy of the same NALs).  Traffic = the packet bytes
read + the output bytes written; the packet table (16 B a packet, read three times), the 44 B a packet and 24 B a piece of scratch
and the 36 B a NAL of output tables are not counted.  Fractions of the 8 TB/s peak.
    python scripts/rtpun_time.py [--gib 16] [--small-gib 2] [--reps 5] [--au-nals 8]"""
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
        yield "S(0x1234, %d) ~10 KiB NALs" % n, g["stream"][: g["stream_bytes"]], n, (1188, 8948)
        del g
        arena, total, idx, n, stream, sb = make_stream(torch, np, ctx, 1024, int(args.small_gib * 2**30))
        del arena, idx
        yield "random payload, ~1 KiB NALs", stream[:sb], n, (1188,)

    def timed(call):
        ctx.enable_timing(True)
        call()                                          # warm-up
        for _ in range(args.reps):
            call()
        ms = sorted(ctx.kernel_ms_back(b) for b in range(args.reps))
        ctx.enable_timing(False)
        return ms

    def report(name, what, ms, traffic, extra):
        med = ms[len(ms) // 2]
        row = dict(stream=name, call=what, kernel_ms_min=round(ms[0], 4), kernel_ms_median=round(med, 4), traffic_bytes=traffic,
                   gbs=round(traffic / med / 1e6, 1), fraction_of_8tbs=round(traffic / med / 1e6 / HBM_PEAK_GBS, 3), **extra)
        rows.append(row)
        print("%-34s %-40s %8.3f ms (min %8.3f)  %7.0f GB/s  %.3f of 8 TB/s (bytes read + bytes written)"
              % (name, what, med, ms[0], row["gbs"], row["fraction_of_8tbs"]), flush=True)
        return med

    for name, raw, n_raw, payloads in shapes():
        ent, _, s = ctx.index_extract(raw, index_cap=n_raw + 16, want_rbsp=False)
        assert len(ent) == n_raw, (len(ent), n_raw)
        # what a receiver would read as AP / FU / PACI goes: hbs_rtp_pack refuses such NALs
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
        nal_len = (lens["end"] - lens["start"]).astype(np.int64)
        first_nal = stream[int(lens["start"][0]):int(lens["end"][0])].cpu().numpy()
        last_nal = stream[int(lens["start"][-1]):int(lens["end"][-1])].cpu().numpy()
        nal_bytes = int(nal_len.sum())
        del lens

        n_aus = (n + args.au_nals - 1) // args.au_nals
        nal_au = (np.arange(n) // args.au_nals).astype(np.uint32)
        d_nal_au = torch.from_numpy(nal_au.view(np.uint8).copy()).to(dev)
        pts = (np.arange(n_aus, dtype=np.uint64) * np.uint64(3003)) & np.uint64((1 << 33) - 1)
        d_pts = torch.from_numpy(pts.view(np.uint8).copy()).to(dev)

        for mp in payloads:
            prm = hbs.rtp_params(max_payload=mp, framing=0, seq=65000, ts_base=12345, ssrc=0xCAFEF00D)
            a = (stream, sb, index, n, d_nal_au, n_aus, d_pts, prm)
            assert ctx.rtp_pack_async(*a, None, None, None, summ) == 0
            plan = ctx.read_summary(summ)
            assert int(plan["error"]) == 0 and int(plan["rbsp_bytes"]) == nal_bytes, plan
            packed_bytes, packets = int(plan["stream_bytes"]), int(plan["nal_count"])
            packed = torch.empty(packed_bytes + 16, dtype=torch.uint8, device=dev)
            nal_off, nal_packet = (torch.empty((n + 1) * 8, dtype=torch.uint8, device=dev) for _ in range(2))

            def pack():
                assert ctx.rtp_pack_async(*a, packed, nal_off, nal_packet, summ, out_cap=packed_bytes) == 0
            pack_ms = timed(pack)
            sm = ctx.read_summary(summ)
            assert int(sm["error"]) == 0 and int(sm["stream_bytes"]) == packed_bytes, sm
            what = "max_payload %d" % mp
            pack_med = report(name, "hbs_rtp_pack " + what, pack_ms, nal_bytes + packed_bytes, dict(max_payload=mp, nals=n, packets=packets))

            # the receiver's table: where every packet begins and how long it is
            off = hbs.rtp_packet_offsets(nal_off.cpu().numpy().view(np.uint64), nal_packet.cpu().numpy().view(np.uint64), mp, 0)
            d_off = torch.from_numpy(off[:-1].view(np.uint8).copy()).to(dev)
            d_size = torch.from_numpy(np.diff(off).view(np.uint8).copy()).to(dev)
            del off, nal_off, nal_packet
            uprm = hbs.rtp_unpack_params(payload_type=96, startcode_bytes=4, flags=hbs.RTPU_MATCH_SSRC, ssrc=0xCAFEF00D)
            b = (packed, packed_bytes, d_off, d_size, packets, uprm)
            assert ctx.rtp_unpack_async(*b, None, None, None, None, summ) == 0
            plan = ctx.read_summary(summ)
            assert int(plan["error"]) == 0 and int(plan["nal_count"]) == n and int(plan["rbsp_bytes"]) == nal_bytes, plan
            assert int(plan["nal_found"]) == packets and int(plan["reserved"][1]) == n_aus and int(plan["reserved"][2]) == 0, plan
            out_bytes = int(plan["stream_bytes"])
            out = torch.empty(out_bytes + 16, dtype=torch.uint8, device=dev)
            index_out = torch.empty(n * 32, dtype=torch.uint8, device=dev)
            nal_au_out = torch.empty(n * 4, dtype=torch.uint8, device=dev)
            au_ts = torch.empty(n_aus * 8, dtype=torch.uint8, device=dev)

            def unpack():
                assert ctx.rtp_unpack_async(*b, out, index_out, nal_au_out, au_ts, summ, out_cap=out_bytes, nal_cap=n, au_cap=n_aus) == 0
            ms = timed(unpack)
            sm = ctx.read_summary(summ)
            assert int(sm["error"]) == 0 and int(sm["stream_bytes"]) == out_bytes and int(sm["nal_count"]) == n, sm
            # what came back: every NAL's length, the AU numbers, the times, the first and the last NAL's bytes
            back = index_out.cpu().numpy().view(hbs.NAL_ENTRY)
            assert np.array_equal((back["end"] - back["start"]).astype(np.int64), nal_len)
            assert np.array_equal(nal_au_out.cpu().numpy().view(np.uint32), nal_au)
            assert np.array_equal(au_ts.cpu().numpy().view(np.uint64), (pts + np.uint64(12345)) & np.uint64(0xFFFFFFFF))
            assert np.array_equal(out[int(back["start"][0]):int(back["end"][0])].cpu().numpy(), first_nal)
            assert np.array_equal(out[int(back["start"][-1]):int(back["end"][-1])].cpu().numpy(), last_nal)
            del back
            med = report(name, "hbs_rtp_unpack " + what, ms, packed_bytes + out_bytes,
                         dict(max_payload=mp, nals=n, packets=packets, packet_bytes=packed_bytes, out_bytes=out_bytes))
            rows[-1]["time_over_pack"] = round(med / pack_med, 3)
            del packed, d_off, d_size
            torch.cuda.empty_cache()

            copy = torch.empty(out_bytes + 16, dtype=torch.uint8, device=dev)
            copy_index = torch.empty(n * 32, dtype=torch.uint8, device=dev)
            rule = ctx.nal_filter()

            def keep_all():
                ctx.filter_annexb_async(out, out_bytes, index_out, n, copy, copy_index, summ, rule=rule)
            filter_ms = timed(keep_all)
            fs = ctx.read_summary(summ)
            assert int(fs["error"]) == 0 and int(fs["nal_count"]) == n, fs
            f_med = report(name, "hbs_filter_annexb keep-all, unpacked", filter_ms, 2 * int(fs["stream_bytes"]), dict(nals=n))
            rows[-2]["time_over_filter"] = round(med / f_med, 3)
            print("%-34s hbs_rtp_unpack %s: %.3f x hbs_rtp_pack's time, %.3f x the filter's" % (name, what, med / pack_med, med / f_med), flush=True)
            del out, index_out, nal_au_out, au_ts, copy, copy_index
            torch.cuda.empty_cache()
        del stream, index, d_nal_au, d_pts
        torch.cuda.empty_cache()
    print(json.dumps({"rtpun_time": rows, "source_digest": hbs.source_digest()}))


if __name__ == "__main__":
    main()
