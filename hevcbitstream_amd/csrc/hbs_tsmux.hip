/*
 * hbs_tsmux.hip -- hbs_ts_mux: the access units of an Annex-B stream -> MPEG transport packets of one PID, one PES packet an
 * AU, a PAT and a PMT where asked for (include/hevcbitstream_amd.h; the packet rule is tsm_packet / tsm_head_byte,
 * hbs_tsmux.h).  The filter's plan shape, then a copy that needs no piece table because the packets have a fixed stride.
 * Five launches, none of which waits for another workgroup:
 *
 *   k_tsm_count   one lane per 4 consecutive AUs, 256 AUs a workgroup: checks the entries and the times; per workgroup the
 *                 sums of ES packets, PSI pairs and ES bytes, and 1 + its lowest bad AU
 *   k_tsm_scan    one workgroup: exclusive scan of those sums over the workgroups (scan_parts, hbs_plan.h); the totals, the
 *                 error, the summary.  A plan-only call ends here
 *   k_tsm_place   the entries once more, now with the offsets: the packet each AU's PES begins in (d_au_packet and scratch)
 *                 and the ES packets in front of it (scratch: the continuity counter)
 *   k_tsm_blocks  one lane per 2048 output packets: binary search of the AU its first packet belongs to
 *   k_tsm_copy    one workgroup per 2048 output packets, in rounds of 256: the AU offsets of the workgroup's range are staged
 *                 in LDS; each round a lane lays one packet out (its AU by binary search of the staged offsets, then the
 *                 rule) and leaves where its ES bytes begin and where they come from; the round's output is then copied in
 *                 the skeleton that hbs_copy16.h describes, its batch loop written out here: the fast path for every aligned
 *                 16-byte chunk that lies wholly inside one packet's ES bytes; the chunks that hold header, adaptation-field,
 *                 PES-header or PSI bytes, the zero bytes of 192- and 204-byte packets, or span two packets -- one in twelve
 *                 at 188 bytes with full packets -- are marked in a bit mask and assembled byte by byte behind them, from the
 *                 rule; the output's last chunk is stored byte-exactly.  Rounds and workgroups begin on 16-byte boundaries of
 *                 the output (256 B is a multiple of 16), so no two write the same chunk.
 *
 * Traffic: the AUs' bytes read once and the output written once; 32 B an AU of the AU table and its times read by each plan
 * pass (64-byte records: a line an AU) and again by the packets' lanes of the copy, from the L2; 8 B an AU of scratch.
 */
#include <hip/hip_runtime.h>
#include "hbs_tsmux.h"
#include "hbs_plan.h"
#include "hbs_copy16.h"

namespace hbs {
namespace {

constexpr int kMT = 256;                                              /* lanes of the copy workgroup              */
constexpr int kRounds = kTsmPacketsPerBlock / kTsmRoundPackets;
constexpr uint32_t kStage = kTsmPacketsPerBlock + 3;                  /* AUs a copy workgroup stages: see k_tsm_copy */
constexpr uint32_t kNone = 0xFFFFFFFFu;
static_assert(kTsmRoundPackets == kMT, "the copy lays one packet out per lane");

struct AuEval {
    TsmAu u;
    uint64_t begin, end;
    bool bad, psi;
};

/* entry k with the end of entry k-1 (0 for k = 0): every check of the call that is about AU k */
__device__ __forceinline__ AuEval eval_au(const TsmArgs& a, uint64_t k, uint64_t prev_end)
{
    const hbs_access_unit* e = a.au + k;
    AuEval r;
    r.begin = e->unit_begin; r.end = e->unit_end;
    const bool irap = (e->flags & HBS_AU_IRAP) != 0;
    const uint64_t pts = a.pts ? a.pts[k] : kTsmNoTime, dts = a.dts ? a.dts[k] : kTsmNoTime;
    r.bad = r.begin > r.end || r.end > a.n || r.begin < prev_end || !tsm_times_ok(pts, dts);
    r.u = tsm_au(r.bad ? 0 : r.end - r.begin, pts, dts, irap, a.flags);
    r.psi = tsm_psi_before(k, irap, a.flags);
    return r;
}

__global__ __launch_bounds__(kTsmPlanLanes) void k_tsm_count(TsmArgs a)
{
    const uint64_t base = (uint64_t)blockIdx.x * kTsmAusPerBlock + (uint64_t)threadIdx.x * kTsmPlanPer;
    uint64_t v[3] = {0, 0, 0};
    uint64_t bad = 0;
    if (base < a.n_aus) {
        uint64_t prev = base ? a.au[base - 1].unit_end : 0;
        for (int i = 0; i < kTsmPlanPer && base + i < a.n_aus; ++i) {
            const AuEval x = eval_au(a, base + i, prev);
            prev = x.end;
            if (x.bad) { if (!bad) bad = base + i + 1; continue; }
            v[0] += tsm_au_packets(x.u); v[1] += x.psi ? 1 : 0; v[2] += x.u.es_bytes;
        }
    }
    bad = block_min_nonzero(bad);
    uint64_t ex[3], tot[3];
    block_scan<3, kTsmPlanLanes>(v, ex, tot);
    if (threadIdx.x == 0) {
        unsigned long long* p = a.part + (uint64_t)blockIdx.x * 8;
        p[0] = tot[0]; p[1] = tot[1]; p[2] = tot[2]; p[3] = bad;
    }
}

__global__ __launch_bounds__(kPlanLanes) void k_tsm_scan(TsmArgs a, uint64_t blocks)
{
    uint64_t carry[3];
    const uint64_t bad = scan_parts<3>(a.part, blocks, carry);
    if (threadIdx.x == 0) {
        const uint64_t es = carry[0], pairs = carry[1], packets = es + 2 * pairs;
        const bool many = packets > 0xFFFFFFFFull;
        const int32_t err = (bad || many) ? HBS_E_ARG : (a.out && packets * a.B > a.out_cap) ? HBS_E_CAPACITY : 0;
        a.ctl[0] = (unsigned long long)(uint32_t)err;
        a.ctl[1] = packets;
        if (!err && a.out) {
            a.au_pkt[a.n_aus] = (uint32_t)packets; a.es_pkt[a.n_aus] = (uint32_t)es;
            if (a.au_packet) a.au_packet[a.n_aus] = (uint32_t)packets;
        }
        hbs_summary s;
        s.nal_count = packets; s.nal_found = a.n_aus; s.rbsp_bytes = carry[2]; s.stream_bytes = many ? 0 : packets * a.B;
        s.stop_reason = 0; s.error = err;
        s.reserved[0] = bad; s.reserved[1] = es; s.reserved[2] = pairs;
        *a.summary = s;
    }
}

__global__ __launch_bounds__(kTsmPlanLanes) void k_tsm_place(TsmArgs a)
{
    if (a.ctl[0] != 0) return;
    const uint64_t base = (uint64_t)blockIdx.x * kTsmAusPerBlock + (uint64_t)threadIdx.x * kTsmPlanPer;
    const bool in = base < a.n_aus;
    uint32_t np[kTsmPlanPer], ps[kTsmPlanPer];          /* the lane's AUs, read once: kept in registers across the scan */
    uint64_t v[2] = {0, 0};
    uint64_t prev = (base && in) ? a.au[base - 1].unit_end : 0;
#pragma unroll
    for (int i = 0; i < kTsmPlanPer; ++i) {
        np[i] = 0; ps[i] = 0;
        if (base + i < a.n_aus) {
            const AuEval x = eval_au(a, base + i, prev);
            prev = x.end;
            np[i] = (uint32_t)tsm_au_packets(x.u); ps[i] = x.psi ? 1u : 0u;
            v[0] += np[i]; v[1] += ps[i];
        }
    }
    uint64_t off[2], tot[2];
    block_scan<2, kTsmPlanLanes>(v, off, tot);
    if (!in) return;
    const unsigned long long* p = a.part + (uint64_t)blockIdx.x * 8;
    off[0] += p[0]; off[1] += p[1];
#pragma unroll
    for (int i = 0; i < kTsmPlanPer; ++i) {
        if (base + i >= a.n_aus) break;
        off[1] += ps[i];
        const uint32_t at = (uint32_t)(off[0] + 2 * off[1]);
        a.es_pkt[base + i] = (uint32_t)off[0];
        a.au_pkt[base + i] = at;
        if (a.au_packet) a.au_packet[base + i] = at;
        off[0] += np[i];
    }
}

__global__ __launch_bounds__(256) void k_tsm_blocks(TsmArgs a)
{
    if (a.ctl[0] != 0) return;
    const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t P = b * kTsmPacketsPerBlock;
    if (b >= a.copy_blocks || P >= a.ctl[1]) return;
    /* the last AU whose PES begins at or in front of P (0 when none does) */
    a.blk_first[b] = (uint32_t)last_le((uint64_t)0, a.n_aus - 1, P, [&](uint64_t k) { return (uint64_t)a.au_pkt[k]; });
}

/* what the bytes in front of a packet's ES bytes are made from */
struct PacketCtx {
    TsmAu u;
    TsmPacket p;
    uint64_t begin;          /* the AU's unit_begin                                                                  */
    uint32_t psi;            /* 0: an ES packet; 1: the PAT, 2: the PMT of a pair                                     */
    uint32_t cc;             /* ES: the packet's number among the call's ES packets + cc_es; PSI: the pair's number  */
};

/* output packet P, whose AU is staged entry r (s_pkt[r] <= P < s_pkt[r + 1]; kNone: P lies in front of the first AU's PES,
 * in the pair in front of it) */
__device__ __forceinline__ void packet_ctx(const TsmArgs& a, const uint32_t* s_pkt, uint64_t a0, uint32_t r, uint64_t P, PacketCtx& c)
{
    if (r == kNone) { c.psi = 1u + (uint32_t)(P + 2u - s_pkt[0]); c.cc = 0; return; }
    const uint64_t k = a0 + r;
    const uint32_t e0 = a.es_pkt[k], e1 = a.es_pkt[k + 1], j = (uint32_t)P - s_pkt[r];
    if (j >= e1 - e0) {                                /* behind the AU's packets: the pair in front of the next AU */
        c.psi = 1u + (j - (e1 - e0));
        c.cc = (s_pkt[r + 1] - e1) / 2u - 1u;
        return;
    }
    c.psi = 0; c.cc = a.cc_es + e0 + j;
    const hbs_access_unit* e = a.au + k;
    c.begin = e->unit_begin;
    c.u = tsm_au(e->unit_end - c.begin, a.pts ? a.pts[k] : kTsmNoTime, a.dts ? a.dts[k] : kTsmNoTime, (e->flags & HBS_AU_IRAP) != 0, a.flags);
    tsm_packet(c.u, j, c.p);
}

/* kB = packet_bytes: the divisions by it and the zero bytes around the 188 fold into constants */
template <int kB>
__global__ __launch_bounds__(kMT) void k_tsm_copy(TsmArgs a)
{
    constexpr uint32_t kLead = kB == 192 ? 4u : 0u;
    constexpr uint32_t kRoundChunks = (uint32_t)kTsmRoundPackets * kB / 16u;
    constexpr int kPerLane = (int)((kRoundChunks + kMT - 1) / kMT);
    static_assert(((uint32_t)kTsmRoundPackets * kB) % 16u == 0, "a round begins on a chunk boundary");
    static_assert(kPerLane <= 32, "the slow chunks of a round are a bit mask");
    /* AUs [a0, a0 + cnt] whose PES may begin in the workgroup's packets [P0, P0 + 2048): the PES of AU a0 + 1 + i begins at
     * P0 + 1 + i or behind (every AU has a packet), and the pair in front of an AU two packets earlier */
    __shared__ uint32_t s_pkt[kStage + 1];
    __shared__ unsigned long long s_delta[kTsmRoundPackets];          /* ES byte at output offset o = src[o + delta]             */
    __shared__ uint32_t s_head[kTsmRoundPackets];                     /* transport bytes in front of the ES bytes (188: PSI)     */
    __shared__ uint32_t s_au[kTsmRoundPackets];                       /* the packet's staged AU (kNone: the pair in front of all) */
    if (a.ctl[0] != 0) return;
    const uint64_t total = a.ctl[1];
    const uint64_t P0 = (uint64_t)blockIdx.x * kTsmPacketsPerBlock;
    if (P0 >= total) return;
    const uint64_t P1 = total - P0 < (uint64_t)kTsmPacketsPerBlock ? total : P0 + kTsmPacketsPerBlock;
    const uint64_t a0 = a.blk_first[blockIdx.x];
    const uint32_t cnt = a.n_aus - a0 < (uint64_t)kStage ? (uint32_t)(a.n_aus - a0) : kStage;
    for (uint32_t i = threadIdx.x; i <= cnt; i += kMT) s_pkt[i] = a.au_pkt[a0 + i];
    __syncthreads();
#pragma unroll 1
    for (int round = 0; round < kRounds; ++round) {
        const uint64_t R0 = P0 + (uint64_t)round * kTsmRoundPackets;
        if (R0 >= P1) break;
        {   /* lane t lays packet R0 + t out */
            const uint64_t P = R0 + threadIdx.x;
            uint32_t head = kTsBytes, r = kNone;
            uint64_t delta = 0;
            if (P < P1) {
                /* the last staged AU whose PES begins at or in front of P */
                if (s_pkt[0] <= P) r = last_le(0u, cnt - 1, P, [&](uint32_t i) { return (uint64_t)s_pkt[i]; });
                PacketCtx c;
                packet_ctx(a, s_pkt, a0, r, P, c);
                if (!c.psi) { head = c.p.head; delta = c.begin + c.p.src_off - (P * kB + kLead + head); }
            }
            s_head[threadIdx.x] = head; s_delta[threadIdx.x] = delta; s_au[threadIdx.x] = r;
        }
        __syncthreads();
        const uint64_t obase = R0 * kB;                               /* a multiple of 16 */
        const uint32_t rbytes = (uint32_t)(P1 - R0 < (uint64_t)kTsmRoundPackets ? P1 - R0 : (uint64_t)kTsmRoundPackets) * kB;
        uint32_t slow = 0;                                            /* chunks done byte by byte, behind the others: bit k */
        /* copy_batches (hbs_copy16.h) written out: with it hbs_ts_mux of a 16 GiB stream ran 19.2 ms in six processes of six,
         * with this loop 16.2 ms in four of six (profiles/r26/copy_time.txt) */
#pragma unroll 1
        for (int b = 0; b < kPerLane; b += kBatch) {
            u32x4 va[kBatch], vb[kBatch];
            uint32_t sh[kBatch];
            bool simple[kBatch];
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                const uint32_t o = 16u * (threadIdx.x + (uint32_t)kMT * (uint32_t)(b + u));
                simple[u] = false; sh[u] = 0;
                va[u] = zero4(); vb[u] = zero4();
                if (b + u < kPerLane && o < rbytes) {
                    const uint32_t p = o / kB, i = o - p * kB;
                    if (i >= kLead + s_head[p] && i + 16u <= kLead + kTsBytes) {
                        simple[u] = true;
                        load16_pair(a.src, obase + o + s_delta[p], va[u], vb[u], sh[u]);
                    } else {
                        slow |= 1u << (b + u);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                const uint32_t o = 16u * (threadIdx.x + (uint32_t)kMT * (uint32_t)(b + u));
                if (simple[u]) arena_store16(a.out + obase + o, realign(va[u], vb[u], sh[u]));
            }
        }
#pragma unroll 1
        while (slow) {
            const uint32_t k = (uint32_t)__builtin_ctz(slow);
            slow &= slow - 1;
            const uint32_t o = 16u * (threadIdx.x + (uint32_t)kMT * k);
            const uint32_t len = rbytes - o < 16u ? rbytes - o : 16u;
            uint64_t clo = 0, chi = 0;
            uint32_t ctx_of = kNone;
            PacketCtx c;
            c.psi = 0; c.cc = 0;
#pragma unroll 1
            for (uint32_t q = 0; q < len; ++q) {
                const uint32_t oo = o + q, p = oo / kB, i = oo - p * kB;
                uint64_t v = 0;                                       /* the bytes around the 188 */
                if (i >= kLead && i < kLead + kTsBytes) {
                    const uint32_t t = i - kLead;
                    if (t >= s_head[p]) {
                        v = a.src[obase + oo + s_delta[p]];
                    } else {
                        if (ctx_of != p) { packet_ctx(a, s_pkt, a0, s_au[p], R0 + p, c); ctx_of = p; }
                        if (c.psi) {
                            v = t == 3u ? (0x10u | (((c.psi == 1u ? a.cc_pat : a.cc_pmt) + c.cc) & 15u))
                                        : ((a.psi.w[c.psi - 1u][t >> 2] >> (8u * (t & 3u))) & 0xFFu);
                        } else {
                            v = tsm_head_byte(c.u, c.p, a.pid, a.pcr_lead, c.cc, t);
                        }
                    }
                }
                pack_byte(clo, chi, q, v);
            }
            store_chunk(a.out + obase + o, clo, chi, len);
        }
        __syncthreads();                                              /* the packets' layout is the next round's */
    }
}

} // namespace

hipError_t launch_ts_mux(const TsmArgs& a, hipStream_t st)
{
    const uint64_t blocks = (a.n_aus + kTsmAusPerBlock - 1) / kTsmAusPerBlock;
    const hipError_t e = begin_launches(a.ev_begin, st);
    if (e != hipSuccess) return e;
    if (blocks) hipLaunchKernelGGL(k_tsm_count, dim3((unsigned)blocks), dim3(kTsmPlanLanes), 0, st, a);
    hipLaunchKernelGGL(k_tsm_scan, dim3(1), dim3(kPlanLanes), 0, st, a, blocks);
    if (a.out && blocks) {
        hipLaunchKernelGGL(k_tsm_place, dim3((unsigned)blocks), dim3(kTsmPlanLanes), 0, st, a);
        if (a.copy_blocks) {
            const dim3 grid((unsigned)a.copy_blocks);
            hipLaunchKernelGGL(k_tsm_blocks, dim3((unsigned)((a.copy_blocks + 255) / 256)), dim3(256), 0, st, a);
            if (a.B == 188) hipLaunchKernelGGL(k_tsm_copy<188>, grid, dim3(kMT), 0, st, a);
            else if (a.B == 192) hipLaunchKernelGGL(k_tsm_copy<192>, grid, dim3(kMT), 0, st, a);
            else hipLaunchKernelGGL(k_tsm_copy<204>, grid, dim3(kMT), 0, st, a);
        }
    }
    return end_launches(a.ev_end, st);
}

} // namespace hbs

extern "C" {

int hbs_ts_mux_psi_host(const hbs_ts_mux_params* params, uint8_t pat188[188], uint8_t pmt188[188])
{
    return hbs::tsm_psi_host(params, pat188, pmt188);
}

uint64_t hbs_ts_mux_au_packets_host(uint64_t es_bytes, int time_fields, int pcr)
{
    return hbs::tsm_au_packets_host(es_bytes, time_fields, pcr);
}

}
