/*
 * hbs_rtp.hip -- hbs_rtp_pack: the NAL units of a stream -> RTP packets by RFC 7798, single NAL unit packets and fragmentation
 * units, the marker bit on the last packet of an access unit (include/hevcbitstream_amd.h; the packet rule is rtp_nal /
 * rtp_head_byte, hbs_rtp.h).  The filter's plan shape per NAL, then a copy that needs no per-packet table because all packets
 * of a NAL but its last have one size.  Five launches, none of which waits for another workgroup:
 *
 *   k_rtp_count   one lane a NAL, 256 NALs a workgroup: checks the entry, reads the NAL's first byte, checks the AU number and
 *                 the time; per workgroup the sums of output bytes, packets, NAL bytes and FU NALs, and 1 + its lowest bad NAL
 *   k_rtp_scan    one workgroup: exclusive scan of those sums over the workgroups (scan_parts, hbs_plan.h); the totals, the
 *                 error, the summary.  A plan-only call ends here
 *   k_rtp_place   the entries once more, now with the offsets: per NAL its output offset, first packet number, source offset,
 *                 length and timestamp with the marker (scratch), d_nal_off and d_nal_packet
 *   k_rtp_tiles   one lane per 64 KiB output tile: binary search of the NAL its first byte lies in
 *   k_rtp_copy    one workgroup per output tile: each lane takes 16-byte output chunks 4 KiB apart and finds the NAL of each
 *                 (the tile's NALs are staged in LDS; more than 512 are read from memory); the packet of the chunk is a
 *                 division by the full packet's size.  The copy is the skeleton of hbs_copy16.h: copy_batches for the chunks
 *                 that lie wholly inside one packet's NAL bytes; a chunk that holds length, RTP header or FU header bytes or
 *                 spans packets or NALs -- two in 75 at 1 200-byte packets -- goes to the list in LDS, and copy_slow_list
 *                 makes its bytes from the rule (chunk_byte).
 *
 * HBS_RTP_AGGREGATE (aggregation packets for groups of small NALs) is a second instance of k_rtp_count, k_rtp_place and
 * k_rtp_copy; the instance without the flag compiles from the statements it had before the flag existed.  In the plan each
 * workgroup finds the groups of its 256 NALs alone (ap_groups): 2 + L scanned over the lanes, next(i) by binary search
 * (rtp_group_next), then ONE LANE WALKS EACH RUN between the starts that are known without walking -- lane 0, the first NAL of an
 * access unit, a NAL that can share a packet with no other and the NAL behind it -- and marks the group starts it meets; the
 * runs are disjoint, so at most 256 steps are taken in all.  (The other way, eight rounds of pointer doubling, needs eight
 * tables of jumps in LDS and marks no faster where access units are short.)  A group's first lane folds the PayloadHdr over its
 * units.  In the copy a unit of an AP is one more kind of NAL: 16 (+ framing) bytes in front of the first unit's bytes, 2 in
 * front of a later unit's; its chunks take the same fast path, and a slow chunk's bytes find their NAL by search, because a
 * unit may have as few as 4 output bytes and a chunk may touch five.
 *
 * Traffic: the NALs' bytes read once and the output written once; 32 B a NAL of the index read by each plan pass, 40 B a NAL of
 * scratch written and read (44 B with HBS_RTP_AGGREGATE), 8 B a tile.
 */
#include <hip/hip_runtime.h>
#include "hbs_rtp.h"
#include "hbs_plan.h"
#include "hbs_copy16.h"

namespace hbs {
namespace {

constexpr int kRT = 256;                                              /* lanes of the copy workgroup             */
constexpr uint32_t kTile = (uint32_t)kRtpTileBytes;
constexpr int kChunks = (int)(kRtpTileBytes / 16 / kRT);              /* 16-byte output chunks a copy lane takes */
constexpr uint32_t kLdsNals = 512;                                    /* NALs a tile stages in LDS; more: read from memory */
constexpr unsigned long long kMarker = 1ull << 32;                    /* rec_tm: the NAL ends its access unit    */
constexpr unsigned long long kKindShift = 62, kLenMask = (1ull << kKindShift) - 1;   /* rec_len with HBS_RTP_AGGREGATE */
constexpr uint32_t kOwn = 0, kApFirst = 1, kApLater = 2;              /* ... its kinds                           */

struct NalEval {
    uint64_t start, L;
    uint32_t ts;
    bool bad, marker;
    RtpNal u;
    uint32_t h0, h1;                                                  /* kAp only: the NAL's header bytes (0, 0 for a bad NAL) */
};

/* entry k: every check of the call that is about NAL k; each thing is checked before it is used */
template <bool kAp>
__device__ __forceinline__ NalEval eval_nal(const RtpArgs& a, uint64_t k)
{
    const hbs_nal_entry* e = a.index + k;
    const uint64_t start = e->start, end = e->end, prev_end = k ? a.index[k - 1].end : 0;
    NalEval r;
    r.start = start; r.L = 0; r.ts = 0;
    r.bad = start > end || end > a.n || start < prev_end;
    if constexpr (!kAp) {
        if (!r.bad) {
            r.L = end - start;
            if (r.L < 2) r.bad = true;
            else if (((a.src[start] >> 1) & 63u) >= 48u) r.bad = true;
        }
    } else {
        r.h0 = r.h1 = 0;
        if (!r.bad) {
            r.L = end - start;
            if (r.L < 2) r.bad = true;
            else {                                                    /* (L >= 2: both header bytes are the stream's) */
                r.h0 = a.src[start]; r.h1 = a.src[start + 1];
                if (((r.h0 >> 1) & 63u) >= 48u) { r.bad = true; r.h0 = r.h1 = 0; }
            }
        }
    }
    uint32_t rel = 0;
    bool au_ok = true;
    r.marker = k + 1 == a.n_nals ? !(a.flags & HBS_RTP_OPEN_END) : false;
    if (a.nal_au) {
        const uint32_t au = a.nal_au[k], first = a.nal_au[0];
        if (k) {
            const uint32_t prev = a.nal_au[k - 1];
            if (au != prev && (uint64_t)au != (uint64_t)prev + 1) au_ok = false;
        }
        rel = au - first;
        if (au < first || (uint64_t)rel >= a.n_aus) au_ok = false;
        if (k + 1 < a.n_nals) r.marker = a.nal_au[k + 1] != au;
    }
    if (!au_ok) { r.bad = true; rel = 0; }
    if (a.pts) {
        const uint64_t t = au_ok ? a.pts[rel] : 0;
        if (t >= kRtpTimeLimit) r.bad = true;
        r.ts = a.ts_base + (uint32_t)t;
    } else {
        r.ts = a.ts_base + rel * a.ts_step;
    }
    r.u = rtp_nal(r.bad ? 2 : r.L, a.q.mp, a.q.fr);
    return r;
}

/* HBS_RTP_AGGREGATE: what the group rule makes of the workgroup's NAL `x` (lane t, NAL k; in: k < n_nals) */
struct ApLane {
    uint32_t kind;                                                    /* kOwn, kApFirst, kApLater                           */
    uint32_t pay;                                                     /* kApFirst: the AP's payload bytes                   */
    uint32_t hdr;                                                     /* kApFirst: rtp_ap_payload_hdr                       */
    bool marker;                                                      /* kApFirst: its last unit ends its access unit       */
    uint64_t out_bytes, packets;                                      /* the lane's share of the output and of the packets  */
};

__device__ __forceinline__ ApLane ap_groups(const RtpArgs& a, uint64_t k, bool in, const NalEval& x)
{
    __shared__ uint32_t s_pre[kRtpNalsPerBlock + 1];                  /* the weights in front of lane t               */
    __shared__ uint32_t s_au[kRtpNalsPerBlock];
    __shared__ uint32_t s_hm[kRtpNalsPerBlock];                       /* h0 | h1 << 8 | marker << 16                  */
    __shared__ uint16_t s_next[kRtpNalsPerBlock];
    __shared__ uint8_t s_known[kRtpNalsPerBlock], s_start[kRtpNalsPerBlock];
    const uint32_t t = threadIdx.x;
    const uint64_t base = k - t, left = a.n_nals - base;              /* (the workgroup has at least one NAL)         */
    const uint32_t hi = left < (uint64_t)kRtpNalsPerBlock ? (uint32_t)left : (uint32_t)kRtpNalsPerBlock;
    const uint32_t w = in ? rtp_ap_weight(x.bad ? 2 : x.L) : 0u;
    uint64_t wv[1] = {w}, ex[1], tot[1];
    block_scan<1, kRtpPlanLanes>(wv, ex, tot);
    s_pre[t] = (uint32_t)ex[0];
    if (t == 0) s_pre[kRtpNalsPerBlock] = (uint32_t)tot[0];
    s_au[t] = in && a.nal_au ? a.nal_au[k] : 0u;
    s_hm[t] = x.h0 | x.h1 << 8 | (x.marker ? 1u << 16 : 0u);
    __syncthreads();
    uint32_t next = t + 1;
    bool known = false;
    if (in) {
        next = rtp_group_next(t, hi, a.q.mp, [&](uint32_t j) { return (uint64_t)s_pre[j]; }, [&](uint32_t j) { return s_au[j]; });
        known = t == 0 || s_au[t] != s_au[t - 1] || rtp_ap_loner(w, a.q.mp) || rtp_ap_loner(s_pre[t] - s_pre[t - 1], a.q.mp);
    }
    s_next[t] = (uint16_t)next;
    s_known[t] = known; s_start[t] = known;
    __syncthreads();
    if (known)
        for (uint32_t j = next; j < hi && !s_known[j]; j = s_next[j]) s_start[j] = 1;
    __syncthreads();
    ApLane r;
    r.kind = kOwn; r.pay = 0; r.hdr = 0; r.marker = false; r.out_bytes = 0; r.packets = 0;
    if (!in) return r;
    if (!s_start[t]) {
        r.kind = kApLater; r.out_bytes = w;
    } else if (next - t >= 2u) {
        r.kind = kApFirst; r.pay = kRtpApHead + (s_pre[next] - s_pre[t]);
        uint32_t acc = kRtpApFoldStart;
        for (uint32_t j = t; j < next; ++j) acc = rtp_ap_fold(acc, s_hm[j] & 0xFFu, (s_hm[j] >> 8) & 0xFFu);
        r.hdr = rtp_ap_payload_hdr(acc);
        r.marker = (s_hm[next - 1] >> 16) != 0;
        r.out_bytes = (uint64_t)a.q.fr + kRtpHeader + kRtpApHead + w; r.packets = 1;
    } else {
        r.out_bytes = x.u.out_bytes; r.packets = x.u.packets;
    }
    return r;
}

template <bool kAp>
__global__ __launch_bounds__(kRtpPlanLanes) void k_rtp_count(RtpArgs a)
{
    const uint64_t k = (uint64_t)blockIdx.x * kRtpNalsPerBlock + threadIdx.x;
    uint64_t v[4] = {0, 0, 0, 0};
    uint64_t bad = 0;
    if constexpr (!kAp) {
        if (k < a.n_nals) {
            const NalEval x = eval_nal<false>(a, k);
            if (x.bad) bad = k + 1;
            else { v[0] = x.u.out_bytes; v[1] = x.u.packets; v[2] = x.L; v[3] = x.u.fu ? 1 : 0; }
        }
    } else {
        const bool in = k < a.n_nals;
        NalEval x;
        x.start = 0; x.L = 0; x.ts = 0; x.bad = false; x.marker = false; x.h0 = x.h1 = 0;
        if (in) x = eval_nal<true>(a, k);
        const ApLane g = ap_groups(a, k, in, x);
        if (in) {
            if (x.bad) bad = k + 1;                                   /* FU NALs, and in the high word the APs */
            else { v[0] = g.out_bytes; v[1] = g.packets; v[2] = x.L; v[3] = (g.kind == kOwn && x.u.fu ? 1ull : 0ull) | (g.kind == kApFirst ? 1ull << 32 : 0ull); }
        }
    }
    bad = block_min_nonzero(bad);
    uint64_t ex[4], tot[4];
    block_scan<4, kRtpPlanLanes>(v, ex, tot);
    if (threadIdx.x == 0) {
        unsigned long long* p = a.part + (uint64_t)blockIdx.x * 8;
        p[0] = tot[0]; p[1] = tot[1]; p[2] = tot[2]; p[3] = tot[3]; p[4] = bad;
    }
}

__global__ __launch_bounds__(kPlanLanes) void k_rtp_scan(RtpArgs a, uint64_t blocks)
{
    uint64_t carry[4];
    const uint64_t bad = scan_parts<4>(a.part, blocks, carry);
    if (threadIdx.x == 0) {
        const uint64_t total = carry[0], packets = carry[1];
        const int32_t err = bad ? HBS_E_ARG : (a.out && total > a.out_cap) ? HBS_E_CAPACITY : 0;
        a.ctl[0] = (unsigned long long)(uint32_t)err;
        a.ctl[1] = total; a.ctl[2] = packets;
        if (!err && a.out) {
            a.rec_out[a.n_nals] = total; a.rec_pkt[a.n_nals] = packets;
            if (a.nal_off) a.nal_off[a.n_nals] = total;
            if (a.nal_packet) a.nal_packet[a.n_nals] = packets;
        }
        hbs_summary s;
        s.nal_count = packets; s.nal_found = a.n_nals; s.rbsp_bytes = carry[2]; s.stream_bytes = total;
        s.stop_reason = 0; s.error = err;
        s.reserved[0] = bad; s.reserved[1] = packets; s.reserved[2] = carry[3];      /* (APs << 32 | FU NALs: both below 2^32) */
        *a.summary = s;
    }
}

template <bool kAp>
__global__ __launch_bounds__(kRtpPlanLanes) void k_rtp_place(RtpArgs a)
{
    if (a.ctl[0] != 0) return;
    const uint64_t k = (uint64_t)blockIdx.x * kRtpNalsPerBlock + threadIdx.x;
    const bool in = k < a.n_nals;
    uint64_t v[2] = {0, 0};
    NalEval x;
    x.start = 0; x.L = 0; x.ts = 0; x.marker = false;
    [[maybe_unused]] ApLane g;
    if constexpr (!kAp) {
        if (in) {
            x = eval_nal<false>(a, k);
            v[0] = x.u.out_bytes; v[1] = x.u.packets;
        }
    } else {
        x.bad = false; x.h0 = x.h1 = 0;
        if (in) x = eval_nal<true>(a, k);
        g = ap_groups(a, k, in, x);
        v[0] = g.out_bytes; v[1] = g.packets;
    }
    uint64_t off[2], tot[2];
    block_scan<2, kRtpPlanLanes>(v, off, tot);
    if (!in) return;
    const unsigned long long* p = a.part + (uint64_t)blockIdx.x * 8;
    off[0] += p[0]; off[1] += p[1];
    if constexpr (kAp) {
        if (g.kind == kApLater) off[1] -= 1;                          /* the packet its group's first unit opened */
        if (g.kind == kApFirst) x.marker = g.marker;
        a.rec_ap[k] = g.pay | g.hdr << 16;
        x.L |= (unsigned long long)g.kind << kKindShift;             /* (L is below 2^46: the output fits out_cap) */
    }
    a.rec_out[k] = off[0]; a.rec_pkt[k] = off[1];
    a.rec_src[k] = x.start; a.rec_len[k] = x.L;
    a.rec_tm[k] = (unsigned long long)x.ts | (x.marker ? kMarker : 0ull);
    if (a.nal_off) a.nal_off[k] = off[0];
    if (a.nal_packet) a.nal_packet[k] = off[1];
}

__global__ __launch_bounds__(256) void k_rtp_tiles(RtpArgs a)
{
    if (a.ctl[0] != 0) return;
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t > a.tiles) return;
    tile_first_of<kTile>(a.rec_out, a.n_nals, a.ctl[1], t, a.tile_first);
}

/* the tile's NALs [j0, j0 + cnt): out(i) = where the packets of NAL j0 + i begin in the output (i = cnt: where they end) */
struct TileNals {
    const unsigned long long* s_out; const unsigned long long* s_src; const unsigned long long* s_len;      /* staged: LDS */
    const unsigned long long* rec_out; const unsigned long long* rec_src; const unsigned long long* rec_len;
    uint64_t j0;
    bool lds;
    __device__ __forceinline__ uint64_t out(uint32_t i) const { return lds ? s_out[i] : rec_out[j0 + i]; }
    __device__ __forceinline__ uint64_t src(uint32_t i) const { return lds ? s_src[i] : rec_src[j0 + i]; }
    __device__ __forceinline__ uint64_t len(uint32_t i) const { return lds ? s_len[i] : rec_len[j0 + i]; }
    /* the last NAL i in [lo, hi] with out(i) <= o (out(lo) <= o holds) */
    __device__ __forceinline__ uint32_t find(uint32_t lo, uint32_t hi, uint64_t o) const
    {
        return last_le(lo, hi, o, [&](uint32_t i) { return out(i); });
    }
};

/* the packet of byte q of an FU NAL's output: q / P */
__device__ __forceinline__ uint64_t packet_of(uint64_t q, uint32_t P)
{
    return q <= 0xFFFFFFFFull ? (uint64_t)((uint32_t)q / P) : q / P;
}

/* output byte `cur` of a chunk that holds bytes in front of a packet's NAL bytes or spans packets or NALs (or ends the
 * output), from the rule; ip: the NAL the chunk's first byte lies in (every NAL has at least 14 output bytes, so the byte lies
 * in that NAL or in one of the two behind it).  Every load is issued whatever the byte turns out to be -- the NAL's two header
 * bytes and its record exist for every NAL -- so that the loads of several bytes a lane are in flight together. */
/* ... with HBS_RTP_AGGREGATE a unit of an AP has as few as 4 output bytes, so the byte lies in NAL ip or in one of the four
 * behind it, of the tile's cnt: found by search */
template <bool kAp>
__device__ __forceinline__ uint32_t chunk_byte(const RtpArgs& a, const TileNals& tn, uint32_t ip, uint32_t cnt, uint64_t cur)
{
    if constexpr (!kAp) {
        ip += cur >= tn.out(ip + 1) ? 1u : 0u;
        ip += cur >= tn.out(ip + 1) ? 1u : 0u;
    } else {
        ip = tn.find(ip, ip + 4u < cnt - 1u ? ip + 4u : cnt - 1u, cur);
        const uint64_t len = tn.len(ip);
        const uint32_t kind = (uint32_t)(len >> kKindShift);
        if (kind != kOwn) {
            const uint64_t S = tn.src(ip);
            const uint32_t q = (uint32_t)(cur - tn.out(ip)), L = (uint32_t)len;      /* (an AP has fewer than 2^16 + 14 bytes) */
            if (kind == kApLater) return q < kRtpApSize ? ((q == 0 ? L >> 8 : L) & 0xFFu) : a.src[S + (q - kRtpApSize)];
            const uint32_t head = rtp_ap_first_head(a.q);
            if (q >= head) return a.src[S + (q - head)];
            const unsigned long long tm = a.rec_tm[tn.j0 + ip], pkt = a.rec_pkt[tn.j0 + ip];
            const uint32_t ap = a.rec_ap[tn.j0 + ip];
            return rtp_ap_head_byte(a.q, (tm & kMarker) != 0, ap & 0xFFFFu, pkt, (uint32_t)tm, ap >> 16, L, q);
        }
    }
    const uint32_t P = rtp_full_packet_bytes(a.q);
    const uint64_t O = tn.out(ip), E = tn.out(ip + 1), S = tn.src(ip);
    const bool fu = (kAp ? tn.len(ip) & kLenMask : tn.len(ip)) > a.q.mp;
    const uint64_t q = cur - O;
    const uint64_t p = fu ? packet_of(q, P) : 0;                     /* the packet of the NAL, where it begins, its bytes */
    const uint64_t pstart = O + p * P;
    const uint64_t plen = fu ? (E - pstart < P ? E - pstart : P) : E - O;
    const uint32_t i = (uint32_t)(cur - pstart), head = rtp_head_bytes(a.q, fu);
    const bool payload = i >= head;
    const uint32_t pay = a.src[S + (payload ? rtp_packet_src(a.q, fu, p) + (i - head) : 0u)];
    const uint32_t h0 = a.src[S], h1 = a.src[S + 1];
    const unsigned long long tm = a.rec_tm[tn.j0 + ip], pkt0 = a.rec_pkt[tn.j0 + ip];
    const uint32_t hb = rtp_head_byte(a.q, fu, p == 0, pstart + plen == E, (tm & kMarker) != 0, plen, pkt0 + p, (uint32_t)tm, h0, h1, payload ? 0u : i);
    return payload ? pay : hb;
}

template <bool kAp>
__global__ __launch_bounds__(kRT) void k_rtp_copy(RtpArgs a)
{
    __shared__ unsigned long long s_out[kLdsNals + 1];
    __shared__ unsigned long long s_src[kLdsNals];
    __shared__ unsigned long long s_len[kLdsNals];
    __shared__ uint32_t s_slow[kTile / 16];           /* the chunks done byte by byte: chunk | its NAL's number in the tile << 12 */
    __shared__ uint32_t s_nslow;
    if (a.ctl[0] != 0) return;
    const uint64_t total = a.ctl[1];
    const uint64_t t0 = (uint64_t)blockIdx.x * kTile;
    if (t0 >= total) return;
    const uint32_t tlen = total - t0 < kTile ? (uint32_t)(total - t0) : kTile;
    const uint64_t j0 = a.tile_first[blockIdx.x], j1 = a.tile_first[blockIdx.x + 1];
    const uint32_t cnt = (uint32_t)(j1 - j0 + 1);     /* NALs [j0, j1]; rec_out[j1 + 1] exists (the total at the end) */
    TileNals tn;
    tn.s_out = s_out; tn.s_src = s_src; tn.s_len = s_len;
    tn.rec_out = a.rec_out; tn.rec_src = a.rec_src; tn.rec_len = a.rec_len;
    tn.j0 = j0; tn.lds = false;
    if (cnt <= kLdsNals) {
        for (uint32_t i = threadIdx.x; i <= cnt; i += kRT) {
            s_out[i] = a.rec_out[j0 + i];
            if (i < cnt) { s_src[i] = a.rec_src[j0 + i]; s_len[i] = a.rec_len[j0 + i]; }
        }
        tn.lds = true;
    }
    if (threadIdx.x == 0) s_nslow = 0;
    __syncthreads();
    const uint32_t P = rtp_full_packet_bytes(a.q), F = a.q.mp - 3u, mp = a.q.mp;
    const uint32_t head_single = rtp_head_bytes(a.q, false), head_fu = rtp_head_bytes(a.q, true);
    [[maybe_unused]] const uint32_t head_ap = rtp_ap_first_head(a.q);
    uint32_t lo = 0;
    copy_batches<kRT, kChunks>(a.src, a.out + t0, tlen,
        [&](uint32_t r, uint32_t& ip, uint64_t& s) {
            const uint64_t o = t0 + r;
            ip = lo = tn.find(lo, cnt - 1, o);
            if (o + 16 > tn.out(lo + 1)) return false;                /* the chunk must end inside the NAL's packets */
            const uint64_t q = o - tn.out(lo), S = tn.src(lo);
            uint64_t len = tn.len(lo);
            [[maybe_unused]] uint32_t kind = kOwn;
            if constexpr (kAp) { kind = (uint32_t)(len >> kKindShift); len &= kLenMask; }
            if (kAp && kind != kOwn) {
                const uint32_t head = kind == kApFirst ? head_ap : kRtpApSize;
                s = S + (q - head);
                return q >= head;
            }
            if (len <= mp) {
                s = S + (q - head_single);
                return q >= head_single;
            }
            const uint64_t p = packet_of(q, P);
            const uint32_t i = (uint32_t)(q - p * P);
            s = S + 2u + p * F + (i - head_fu);
            return i >= head_fu && i + 16u <= P;
        },
        [&](uint32_t r, uint32_t ip) { slow_push<kTile>(s_slow, s_nslow, r, ip); });
    __syncthreads();
    copy_slow_list<kRT>(s_slow, s_nslow, a.out, t0, tlen,
                        [&](uint32_t ip, uint64_t cur) { return chunk_byte<kAp>(a, tn, ip, cnt, cur); });
}

} // namespace

/* the call's launches with (kAp) and without HBS_RTP_AGGREGATE */
template <bool kAp>
static void launch_rtp_kernels(const RtpArgs& a, uint64_t blocks, hipStream_t st)
{
    if (blocks) hipLaunchKernelGGL(k_rtp_count<kAp>, dim3((unsigned)blocks), dim3(kRtpPlanLanes), 0, st, a);
    hipLaunchKernelGGL(k_rtp_scan, dim3(1), dim3(kPlanLanes), 0, st, a, blocks);
    if (a.out && blocks) {
        hipLaunchKernelGGL(k_rtp_place<kAp>, dim3((unsigned)blocks), dim3(kRtpPlanLanes), 0, st, a);
        if (a.tiles) {
            hipLaunchKernelGGL(k_rtp_tiles, dim3((unsigned)((a.tiles + 1 + 255) / 256)), dim3(256), 0, st, a);
            hipLaunchKernelGGL(k_rtp_copy<kAp>, dim3((unsigned)a.tiles), dim3(kRT), 0, st, a);
        }
    }
}

hipError_t launch_rtp_pack(const RtpArgs& a, hipStream_t st)
{
    const uint64_t blocks = (a.n_nals + kRtpNalsPerBlock - 1) / kRtpNalsPerBlock;
    const hipError_t e = begin_launches(a.ev_begin, st);
    if (e != hipSuccess) return e;
    if (a.flags & HBS_RTP_AGGREGATE) launch_rtp_kernels<true>(a, blocks, st);
    else launch_rtp_kernels<false>(a, blocks, st);
    return end_launches(a.ev_end, st);
}

} // namespace hbs

extern "C" {

uint64_t hbs_rtp_nal_packets_host(uint64_t nal_bytes, int max_payload)
{
    return hbs::rtp_nal_packets_host(nal_bytes, max_payload);
}

int hbs_rtp_packet_host(const uint8_t* pkt, uint64_t n, hbs_rtp_packet* out)
{
    return hbs::rtp_packet_host(pkt, n, out);
}

}
