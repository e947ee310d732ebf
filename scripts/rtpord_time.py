#!/usr/bin/env python3
"""Kernel time of hbs_rtp_order (the library's HIP events around all of a call's launches, hbs_ctx_kernel_ms) on the packet table
of hbs_rtp_pack (max_payload 1188, packets back to back): the bench stream -- S(0x1234, n) of ~10 KiB NALs, 16 GiB by default,
about 15.4 M packets -- and a stream of ~1 KiB NALs (scripts/nal_sweep.py's shape, 2 GiB by default).  Three arrival orders:
(a) the in-order table, (b) the table shuffled inside a window of 16 (a stable sort on position + random(0..16)) with 1 % of the
packets lost and 1 % arriving twice, (c) the same with HBS_RTPO_AFTER behind the sequence number in front of the first packet.
Next to it, in the same process: hbs_rtp_unpack on the in-order table and on the table hbs_rtp_order made of (b).  As in
scripts/rtpun_time.py, NALs whose type is 48 or above are filtered out before they are packed.  The call reads 16 B of table and
one 16-byte header granule (two where the header straddles) a packet and no payload byte; no traffic figure is derived.
    python scripts/rtpord_time.py [--gib 16] [--small-gib 2] [--reps 5] [--au-nals 8] [--window 16]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
K = 1 << 48
SEQ0 = 65000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=16.0)
    ap.add_argument("--small-gib", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--au-nals", type=int, default=8)
    ap.add_argument("--window", type=int, default=16)
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

    def report(name, what, ms, extra):
        med = ms[len(ms) // 2]
        rows.append(dict(stream=name, call=what, kernel_ms_min=round(ms[0], 4), kernel_ms_median=round(med, 4), **extra))
        print("%-34s %-58s %8.3f ms (min %8.3f)" % (name, what, med, ms[0]), flush=True)
        return med

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(dev)

    for name, raw, n_raw in shapes():
        ent, _, s = ctx.index_extract(raw, index_cap=n_raw + 16, want_rbsp=False)
        assert len(ent) == n_raw, (len(ent), n_raw)
        d_idx = up(ent)
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
        n_aus = (n + args.au_nals - 1) // args.au_nals
        d_nal_au = up((np.arange(n) // args.au_nals).astype(np.uint32))
        d_pts = up((np.arange(n_aus, dtype=np.uint64) * np.uint64(3003)) & np.uint64((1 << 33) - 1))

        mp = 1188
        prm = hbs.rtp_params(max_payload=mp, framing=0, seq=SEQ0, ts_base=12345, ssrc=0xCAFEF00D)
        a = (stream, sb, index, n, d_nal_au, n_aus, d_pts, prm)
        assert ctx.rtp_pack_async(*a, None, None, None, summ) == 0
        plan = ctx.read_summary(summ)
        assert int(plan["error"]) == 0, plan
        packed_bytes, packets = int(plan["stream_bytes"]), int(plan["nal_count"])
        packed = torch.empty(packed_bytes + 16, dtype=torch.uint8, device=dev)
        nal_off, nal_packet = (torch.empty((n + 1) * 8, dtype=torch.uint8, device=dev) for _ in range(2))
        assert ctx.rtp_pack_async(*a, packed, nal_off, nal_packet, summ, out_cap=packed_bytes) == 0
        assert int(ctx.read_summary(summ)["error"]) == 0
        off = hbs.rtp_packet_offsets(nal_off.cpu().numpy().view(np.uint64), nal_packet.cpu().numpy().view(np.uint64), mp, 0)
        t_off, t_size = off[:-1].copy(), np.diff(off)
        del off, nal_off, nal_packet, stream, index, d_nal_au, d_pts
        torch.cuda.empty_cache()

        # (b): what arrives -- 1 % lost, the rest shuffled inside the window, 1 % a second time up to a window behind their first
        rng = np.random.default_rng(17)
        pos = np.arange(packets)
        there = rng.random(packets) >= 0.01
        there[0] = there[-1] = True
        key = pos + rng.integers(0, args.window + 1, size=packets)
        twice = there & (rng.random(packets) < 0.01)
        sent = np.concatenate([pos[there], pos[twice]])
        keys = np.concatenate([key[there], key[twice] + rng.integers(1, args.window + 1, size=int(twice.sum()))])
        arrival = sent[np.argsort(keys, kind="stable")]
        lost, dups = int(packets - there.sum()), int(twice.sum())
        del pos, key, keys, sent

        uprm = hbs.rtp_unpack_params(payload_type=96, startcode_bytes=4, flags=hbs.RTPU_MATCH_SSRC, ssrc=0xCAFEF00D)

        def unpack_on(d_off, d_size, count):
            b = (packed, packed_bytes, d_off, d_size, count, uprm)
            assert ctx.rtp_unpack_async(*b, None, None, None, None, summ) == 0
            plan = ctx.read_summary(summ)
            assert int(plan["error"]) == 0, plan
            out_bytes, nals, aus = int(plan["stream_bytes"]), int(plan["nal_count"]), int(plan["reserved"][1])
            out = torch.empty(out_bytes + 16, dtype=torch.uint8, device=dev)
            index_out = torch.empty(max(nals, 1) * 32, dtype=torch.uint8, device=dev)
            nal_au_out = torch.empty(max(nals, 1) * 4, dtype=torch.uint8, device=dev)
            au_ts = torch.empty(max(aus, 1) * 8, dtype=torch.uint8, device=dev)

            def unpack():
                assert ctx.rtp_unpack_async(*b, out, index_out, nal_au_out, au_ts, summ, out_cap=out_bytes, nal_cap=nals, au_cap=aus) == 0
            ms = timed(unpack)
            sm = ctx.read_summary(summ)
            assert int(sm["error"]) == 0 and int(sm["stream_bytes"]) == out_bytes, sm
            del out, index_out, nal_au_out, au_ts
            torch.cuda.empty_cache()
            return ms, sm

        d_off, d_size = up(t_off), up(t_size)
        ms, sm = unpack_on(d_off, d_size, packets)
        assert int(sm["nal_count"]) == n and int(sm["reserved"][2]) == 0, sm
        unpack_med = report(name, "hbs_rtp_unpack, the in-order table", ms, dict(packets=packets, nals=n))

        cases = (("(a) in order", None, 0), ("(b) window %d, 1 %% lost, 1 %% twice" % args.window, arrival, 0),
                 ("(c) as (b), HBS_RTPO_AFTER", arrival, hbs.RTPO_AFTER))
        for what, order, flags in cases:
            count = packets if order is None else len(order)
            if order is not None:
                d_off, d_size = up(t_off[order]), up(t_size[order])
            oprm = hbs.rtp_order_params(payload_type=96, flags=flags | hbs.RTPO_MATCH_SSRC, ssrc=0xCAFEF00D, max_span=packets,
                                        after_ext=K + SEQ0 - 1 if flags else 0)
            o = (packed, packed_bytes, d_off, d_size, count, oprm)
            assert ctx.rtp_order_async(*o, None, None, None, None, summ) == 0
            plan = ctx.read_summary(summ)
            want_lost, want_dups = (0, 0) if order is None else (lost, dups)
            assert int(plan["error"]) == 0 and int(plan["nal_found"]) == count and int(plan["nal_count"]) == packets - want_lost, plan
            assert int(plan["stream_bytes"]) == packets and int(plan["reserved"][1]) == want_lost and int(plan["reserved"][2]) >> 32 == want_dups, plan
            assert int(plan["rbsp_bytes"]) == K + SEQ0 + packets - 1, plan
            kept = int(plan["nal_count"])
            o_off, o_size, o_ext = (torch.empty(kept * 8, dtype=torch.uint8, device=dev) for _ in range(3))
            o_src = torch.empty(kept * 4, dtype=torch.uint8, device=dev)

            def order_call():
                assert ctx.rtp_order_async(*o, o_off, o_size, o_src, o_ext, summ, out_cap=kept) == 0
            ms = timed(order_call)
            sm = ctx.read_summary(summ)
            assert int(sm["error"]) == 0 and int(sm["nal_count"]) == kept, sm
            # what came out: the sender's order, each packet once
            src = o_src.cpu().numpy().view(np.uint32)
            sender = src if order is None else order[src]
            want = np.arange(packets) if order is None else np.flatnonzero(there)
            assert np.array_equal(sender, want)
            assert np.array_equal(o_ext.cpu().numpy().view(np.uint64), (K + SEQ0 + want).astype(np.uint64))
            assert np.array_equal(o_off.cpu().numpy().view(np.uint64), t_off[want])
            moved = int(sm["reserved"][2]) & 0xFFFFFFFF
            med = report(name, "hbs_rtp_order " + what, ms, dict(packets=count, kept=kept, lost=want_lost, duplicates=want_dups, moved=moved))
            rows[-1]["time_over_unpack_in_order"] = round(med / unpack_med, 4)
            print("%-34s hbs_rtp_order %s: %.4f x hbs_rtp_unpack's time on the in-order table; %d of %d kept packets moved"
                  % (name, what, med / unpack_med, moved, kept), flush=True)
            if order is not None and not flags:
                ms, sm = unpack_on(o_off, o_size, kept)
                report(name, "hbs_rtp_unpack, the table hbs_rtp_order made of (b)", ms,
                       dict(packets=kept, nals=int(sm["nal_count"]), dropped=int(sm["reserved"][2]) & 0xFFFFFFFF, breaks=int(sm["reserved"][2]) >> 32))
            del o_off, o_size, o_ext, o_src
        del packed, d_off, d_size
        torch.cuda.empty_cache()
    print(json.dumps({"rtpord_time": rows, "source_digest": hbs.source_digest()}))


if __name__ == "__main__":
    main()
