/*
 * hbs_ts.hip -- hbs_ts_demux: the packets of one PID of an MPEG transport stream -> their elementary-stream bytes back to
 * back, and the table of PES packets begun (include/hevcbitstream_amd.h; the packet rule is ts_classify, hbs_ts.h).  The
 * filter's plan shape, then a copy that needs no table because the packets have a fixed stride.  Four launches, none of which
 * waits for another workgroup:
 *
 *   k_ts_count   one lane per 8 consecutive packets, 2048 packets a workgroup: each lane reads the header bytes its
 *                packets' classes need.  Per workgroup, in two halves -- in front of and from its own first PES start on --
 *                the ES bytes, packets of the PID, skipped packets, PES starts and continuity breaks; the cc of its first and
 *                last packet with ES bytes; the lowest fault (the block record below)
 *   k_ts_scan    one workgroup: the block of the stream's first PES start, then 256 blocks a pass: what of each block counts
 *                ("behind the stream's first PES start"), the continuity check joined across blocks, exclusive sums of output
 *                bytes and PES starts; totals, the error, the summary.  A plan-only call ends here
 *   k_ts_place   (with d_pes) the packets once more, now with the offsets: the PES table
 *   k_ts_copy    one workgroup per 2048 packets, in rounds of 256: the round's source span (256 B bytes) is loaded as aligned
 *                16-byte granules into an LDS image, its packets are classified FROM the image (one lane each) and their ES
 *                lengths scanned; every aligned 16-byte chunk of the round's output range is then put together from the image
 *                -- the packet by binary search of the in-LDS offsets; a chunk inside one packet's run as five dwords and
 *                alignbyte, one that spans packets byte by byte -- and stored whole; the partial chunks at the two ends of
 *                the range are stored byte-exactly (store_chunk), so neighbouring rounds and workgroups never write the
 *                same byte.  The chunk helpers are hbs_copy16.h, the workgroup scans hbs_plan.h.
 *
 * Traffic: the stream read once by the copy; the plan passes read header bytes only (a cache line in front of each 188 bytes,
 * twice, three times with d_pes); 64 B a block of scratch.
 */
#include <hip/hip_runtime.h>
#include "hbs_ts.h"
#include "hbs_plan.h"
#include "hbs_copy16.h"

namespace hbs {
namespace {

constexpr int kTT = 256;                                          /* lanes of every workgroup here            */
constexpr int kTPer = kTsPacketsPerBlock / kTT;                   /* consecutive packets a plan lane takes    */
constexpr int kRounds = kTsPacketsPerBlock / kTsRoundPackets;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kImageBytesTs = kTsRoundPackets * 204u + 32u;   /* the widest packets, and room for the dword reads behind a run */
static_assert(kTsRoundPackets == kTT, "the copy classifies one packet per lane");

/* the block record: 16 words per block of 2048 packets, written by k_ts_count (0..11) and k_ts_scan (12..15) */
enum : int {
    kPFrontEs = 0, kPBehindEs, kPBehindPes, kPFrontPid, kPBehindPid, kPFrontSkip, kPBehindSkip, kPFrontBrk, kPBehindBrk,
    kPFirstPes,       /* the block's first PES start, 0..2047 (kNone: none); "front" is what lies in front of it            */
    kPCc,             /* packets with ES bytes: bit 0 any, 4..7 cc of the first, 8 its discontinuity_indicator, 12..15 cc of
                         the last, 16: the first PES start breaks continuity against the packet in front of it IN the block */
    kPFault,          /* 1 + the block's lowest faulty packet (0: none)                                                     */
    kPOutLo, kPOutHi, /* output offset of the block's first ES byte                                                         */
    kPPesBase,        /* PES starts in front of the block                                                                   */
    kPLiveEs          /* ES bytes of the block that are output                                                              */
};

/* a packet's bytes in device memory: plain byte loads, every one of them inside the packet */
__device__ __forceinline__ void classify_packet(const TsArgs& a, uint64_t p, hbs_ts_packet& r)
{
    ts_classify(TsByteReader{a.ts + p * a.B + a.lead}, a.pid, r);
}

/* a continuity break at a packet with ES bytes, given the one in front */
__device__ __forceinline__ bool cc_breaks(uint32_t prev_cc, uint32_t cc, bool discontinuity)
{
    return cc != ((prev_cc + 1u) & 15u) && !discontinuity;
}

__global__ __launch_bounds__(kTT) void k_ts_count(TsArgs a)
{
    __shared__ uint32_t s_sum[9];              /* kPFrontEs .. kPBehindBrk */
    __shared__ uint32_t s_first_pes, s_fault, s_first_cc, s_last_cc, s_at_pes;
    const uint32_t j0 = threadIdx.x * kTPer;                          /* the lane's first packet, in the block */
    const uint64_t base = (uint64_t)blockIdx.x * kTsPacketsPerBlock + j0;
    if (threadIdx.x < 9) s_sum[threadIdx.x] = 0;
    if (threadIdx.x == 0) { s_first_pes = kNone; s_fault = kNone; s_first_cc = kNone; s_last_cc = 0; s_at_pes = 0; }
    /* per packet: bits 0..2 class + 1 (0: past the end), 3 discontinuity, 4..7 cc, 8..15 ES bytes */
    uint32_t info[kTPer];
    uint32_t my_pes = kNone, my_fault = kNone;
    uint32_t last_key = 0;                                            /* ((lane + 1) << 4 | cc) of the lane's last packet with ES bytes */
#pragma unroll
    for (int i = 0; i < kTPer; ++i) {
        info[i] = 0;
        if (base + i < a.packets) {
            hbs_ts_packet r;
            classify_packet(a, base + i, r);
            info[i] = (uint32_t)(r.cls + 1) | ((r.flags & HBS_TS_DISCONTINUITY) ? 8u : 0u) | (r.cc << 4) | (r.es_len << 8);
            if (r.cls == HBS_TS_FAULT && my_fault == kNone) my_fault = j0 + i + 1;
            if (r.cls == HBS_TS_PES_START && my_pes == kNone) my_pes = j0 + i;
            if (ts_has_es(r.cls)) last_key = ((threadIdx.x + 1u) << 4) | r.cc;
        }
    }
    __syncthreads();
    if (my_pes != kNone) atomicMin(&s_first_pes, my_pes);
    if (my_fault != kNone) atomicMin(&s_fault, my_fault);
    uint32_t prev, any;                                               /* the last packet with ES bytes in front of the lane */
    block_excl_max<uint32_t, 1, kTT>(&last_key, &prev, &any);
    const uint32_t F = s_first_pes;
    uint32_t sum[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < kTPer; ++i) {
        const int32_t cls = (int32_t)(info[i] & 7u) - 1;
        if (info[i] == 0 || cls == HBS_TS_OTHER || cls == HBS_TS_FAULT) continue;
        const uint32_t j = j0 + i, cc = (info[i] >> 4) & 15u;
        const bool behind = j >= F;
        sum[behind ? kPBehindPid : kPFrontPid] += 1;
        if (cls == HBS_TS_SKIPPED) sum[behind ? kPBehindSkip : kPFrontSkip] += 1;
        if (!ts_has_es(cls)) continue;
        sum[behind ? kPBehindEs : kPFrontEs] += info[i] >> 8;
        if (cls == HBS_TS_PES_START) sum[kPBehindPes] += 1;
        if (prev) {
            if (cc_breaks(prev & 15u, cc, (info[i] & 8u) != 0)) {
                if (j == F) s_at_pes = 1;                              /* (one lane at most) */
                else sum[behind ? kPBehindBrk : kPFrontBrk] += 1;
            }
        } else {
            s_first_cc = cc | ((info[i] & 8u) ? 16u : 0u);            /* the block's first: judged by the scan (one lane at most) */
        }
        prev = ((threadIdx.x + 1u) << 4) | cc;
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) if (sum[q]) atomicAdd(&s_sum[q], sum[q]);
    if (last_key) atomicMax(&s_last_cc, last_key);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t* w = a.part + (uint64_t)blockIdx.x * 16;
#pragma unroll
        for (int q = 0; q < 9; ++q) w[q] = s_sum[q];
        w[kPFirstPes] = F;
        w[kPCc] = s_last_cc ? (1u | ((s_first_cc & 15u) << 4) | ((s_first_cc & 16u) << 4) | ((s_last_cc & 15u) << 12) | (s_at_pes << 16)) : 0u;
        w[kPFault] = s_fault == kNone ? 0u : s_fault;
    }
}

__global__ __launch_bounds__(kTT) void k_ts_scan(TsArgs a, uint32_t blocks)
{
    __shared__ uint32_t s_g;
    __shared__ unsigned long long s_fault, s_tot[3];                  /* skipped, packets of the PID, breaks */
    if (threadIdx.x == 0) { s_g = kNone; s_fault = ~0ull; s_tot[0] = s_tot[1] = s_tot[2] = 0; }
    __syncthreads();
    {   /* the block of the stream's first PES start; the lowest fault */
        uint32_t g = kNone;
        uint64_t fault = ~0ull;
        for (uint32_t i = threadIdx.x; i < blocks; i += kTT) {
            const uint32_t* w = a.part + (uint64_t)i * 16;
            if (g == kNone && w[kPFirstPes] != kNone) g = i;
            if (fault == ~0ull && w[kPFault]) fault = (uint64_t)i * kTsPacketsPerBlock + w[kPFault];
        }
        if (g != kNone) atomicMin(&s_g, g);
        if (fault != ~0ull) atomicMin(&s_fault, (unsigned long long)fault);
    }
    __syncthreads();
    const uint32_t g = s_g;
    const uint64_t fault = s_fault == ~0ull ? 0 : s_fault;
    uint64_t carry_es = 0, carry_pes = 0;
    uint32_t carry_cc = 0;                                            /* 16 | cc of the last output packet so far (0: none) */
    uint64_t skipped = 0, of_pid = 0, breaks = 0;
    for (uint32_t seg = 0; seg < blocks; seg += kTT) {
        const uint32_t i = seg + threadIdx.x;
        const bool in = i < blocks;
        uint32_t* w = a.part + (uint64_t)(in ? i : 0) * 16;
        uint64_t es = 0, pes = 0;
        uint32_t cc = 0;
        bool joins = false;                                           /* the block's first packet with ES bytes is output, and not the stream's first */
        if (in) {
            cc = w[kPCc];
            of_pid += w[kPFrontPid] + w[kPBehindPid];
            if (g == kNone || i < g) {
                skipped += w[kPFrontPid] + w[kPBehindPid];
                cc = 0;
            } else if (i == g) {
                es = w[kPBehindEs]; pes = w[kPBehindPes];
                skipped += w[kPFrontPid] + w[kPBehindSkip];
                breaks += w[kPBehindBrk];
            } else {
                es = (uint64_t)w[kPFrontEs] + w[kPBehindEs]; pes = w[kPBehindPes];
                skipped += w[kPFrontSkip] + w[kPBehindSkip];
                breaks += w[kPFrontBrk] + w[kPBehindBrk] + ((cc >> 16) & 1u);
                joins = (cc & 1u) != 0;
            }
        }
        uint64_t ex_es, tot_es, ex_pes, tot_pes;
        block_scan<1, kTT>(&es, &ex_es, &tot_es);
        block_scan<1, kTT>(&pes, &ex_pes, &tot_pes);
        uint32_t before, last_all;
        const uint32_t key = (cc & 1u) ? (((threadIdx.x + 1u) << 5) | 16u | ((cc >> 12) & 15u)) : 0u;
        block_excl_max<uint32_t, 1, kTT>(&key, &before, &last_all);
        uint32_t prev = before & 31u;
        if (!prev) prev = carry_cc;
        if (joins && prev && cc_breaks(prev & 15u, (cc >> 4) & 15u, ((cc >> 8) & 1u) != 0)) breaks += 1;
        if (in) {
            const uint64_t o = carry_es + ex_es;
            w[kPOutLo] = (uint32_t)o; w[kPOutHi] = (uint32_t)(o >> 32);
            w[kPPesBase] = (uint32_t)(carry_pes + ex_pes);
            w[kPLiveEs] = (uint32_t)es;
        }
        carry_es += tot_es; carry_pes += tot_pes;
        if (last_all) carry_cc = last_all & 31u;
    }
    if (skipped) atomicAdd(&s_tot[0], (unsigned long long)skipped);
    if (of_pid) atomicAdd(&s_tot[1], (unsigned long long)of_pid);
    if (breaks) atomicAdd(&s_tot[2], (unsigned long long)breaks);
    __syncthreads();
    if (threadIdx.x == 0) {
        const bool run = a.out != nullptr;
        const int32_t err = fault ? HBS_E_ARG : (run && (carry_es > a.out_cap || (a.pes && carry_pes > a.pes_cap))) ? HBS_E_CAPACITY : 0;
        a.ctl[0] = (unsigned long long)(uint32_t)err;
        a.ctl[1] = carry_es; a.ctl[2] = carry_pes;
        a.ctl[3] = g == kNone ? ~0ull : (unsigned long long)g * kTsPacketsPerBlock + a.part[(uint64_t)g * 16 + kPFirstPes];
        hbs_summary s;
        s.nal_count = carry_pes; s.nal_found = s_tot[1]; s.rbsp_bytes = 0; s.stream_bytes = carry_es;
        s.stop_reason = 0; s.error = err;
        s.reserved[0] = fault; s.reserved[1] = s_tot[2]; s.reserved[2] = s_tot[0];
        *a.summary = s;
    }
}

__global__ __launch_bounds__(kTT) void k_ts_place(TsArgs a)
{
    if (a.ctl[0] != 0) return;
    const uint64_t first = a.ctl[3];
    const uint32_t* w = a.part + (uint64_t)blockIdx.x * 16;
    if (first == ~0ull || (w[kPLiveEs] == 0 && w[kPBehindPes] == 0)) return;
    const uint64_t base = (uint64_t)blockIdx.x * kTsPacketsPerBlock + (uint64_t)threadIdx.x * kTPer;
    uint64_t es = 0, pes = 0;
#pragma unroll 1
    for (int i = 0; i < kTPer; ++i) {
        const uint64_t p = base + i;
        if (p >= a.packets || p < first) continue;
        hbs_ts_packet r;
        classify_packet(a, p, r);
        if (ts_has_es(r.cls)) { es += r.es_len; pes += r.cls == HBS_TS_PES_START ? 1 : 0; }
    }
    uint64_t o, k, tot;
    block_scan<1, kTT>(&es, &o, &tot);
    block_scan<1, kTT>(&pes, &k, &tot);
    o += ((uint64_t)w[kPOutHi] << 32) | w[kPOutLo];
    k += w[kPPesBase];
    if (!pes) return;
#pragma unroll 1
    for (int i = 0; i < kTPer; ++i) {
        const uint64_t p = base + i;
        if (p >= a.packets || p < first) continue;
        hbs_ts_packet r;
        classify_packet(a, p, r);
        if (!ts_has_es(r.cls)) continue;
        if (r.cls == HBS_TS_PES_START) {
            unsigned long long* e = reinterpret_cast<unsigned long long*>(a.pes + k);
            e[0] = o; e[1] = r.pts; e[2] = r.dts;
            e[3] = (unsigned long long)(uint32_t)p | ((unsigned long long)r.flags << 32);
            k += 1;
        }
        o += r.es_len;
    }
}

__global__ __launch_bounds__(kTT) void k_ts_copy(TsArgs a)
{
    __shared__ u32x4 s_img4[(kImageBytesTs + 15) / 16];
    __shared__ uint32_t s_off[kTsRoundPackets + 1];                   /* round-relative output offset of each packet's run */
    __shared__ uint32_t s_src[kTsRoundPackets];                       /* where the run begins in the image                 */
    if (a.ctl[0] != 0) return;
    const uint32_t* w = a.part + (uint64_t)blockIdx.x * 16;
    if (w[kPLiveEs] == 0) return;
    const uint64_t first = a.ctl[3];
    const uint8_t* img = reinterpret_cast<const uint8_t*>(s_img4);
    const uint32_t* img32 = reinterpret_cast<const uint32_t*>(s_img4);
    uint64_t obase = ((uint64_t)w[kPOutHi] << 32) | w[kPOutLo];
#pragma unroll 1
    for (int round = 0; round < kRounds; ++round) {
        const uint64_t p0 = (uint64_t)blockIdx.x * kTsPacketsPerBlock + (uint64_t)round * kTsRoundPackets;
        if (p0 >= a.packets) break;
        const uint64_t s0 = p0 * a.B;                                 /* a multiple of 256 B: on a granule's boundary */
        const uint64_t left = a.n - s0, span = (uint64_t)kTsRoundPackets * a.B;
        const uint32_t bytes = (uint32_t)(left < span ? left : span);
        const uint32_t granules = (bytes + 15u) / 16u;                /* each holds a byte of the stream */
        for (uint32_t q = threadIdx.x; q < granules; q += kTT)
            s_img4[q] = stream_load16(reinterpret_cast<const u32x4*>(a.ts + s0) + q);
        __syncthreads();
        const uint64_t p = p0 + threadIdx.x;
        uint32_t len = 0, src = 0;
        if (p < a.packets && p >= first) {
            hbs_ts_packet r;
            const uint32_t at = threadIdx.x * a.B + a.lead;
            ts_classify(TsByteReader{img + at}, a.pid, r);
            if (ts_has_es(r.cls)) { len = r.es_len; src = at + r.es_off; }
        }
        const uint64_t len64 = len;
        uint64_t off64, tot64;
        block_scan<1, kTT>(&len64, &off64, &tot64);
        const uint32_t off = (uint32_t)off64, total = (uint32_t)tot64;
        s_off[threadIdx.x] = off; s_src[threadIdx.x] = src;
        if (threadIdx.x == 0) s_off[kTsRoundPackets] = total;
        __syncthreads();
        /* the aligned 16-byte chunks of the output range [obase, obase + total) */
        const uint32_t head = (uint32_t)(obase & 15u);
        const uint32_t chunks = (head + total + 15u) / 16u;
        for (uint32_t c = threadIdx.x; c < chunks && total; c += kTT) {
            const uint32_t lo = c ? 16u * c - head : 0u;
            const uint32_t hi = 16u * c + 16u - head < total ? 16u * c + 16u - head : total;
            /* the packet the chunk's first byte comes from: the last j with s_off[j] <= lo.  That is the first j with
             * s_off[j + 1] > lo, the packet whose run holds byte lo, runs of no bytes in front of it included: s_off does
             * not decrease and lo < total = s_off[256], so the offsets <= lo are s_off[0 .. j] and no others */
            uint32_t j = last_le(0u, (uint32_t)kTsRoundPackets - 1u, lo, [&](uint32_t i) { return s_off[i]; });
            uint8_t* dst = a.out + obase + lo;
            if (hi - lo == 16u && s_off[j + 1] - lo >= 16u) {
                const uint32_t at = s_src[j] + (lo - s_off[j]);
                arena_store16(dst, realign(img32 + (at >> 2), at & 3u));
                continue;
            }
            uint64_t clo = 0, chi = 0;
            uint32_t end = s_off[j + 1], at = s_src[j] + (lo - s_off[j]);
#pragma unroll 1
            for (uint32_t q = lo; q < hi; ++q) {
                while (q >= end) { j += 1; end = s_off[j + 1]; at = s_src[j]; }     /* (runs of no bytes are passed over) */
                pack_byte(clo, chi, q - lo, img[at++]);
            }
            store_chunk(dst, clo, chi, hi - lo);
        }
        obase += total;
        __syncthreads();                                              /* the image and the offsets are the next round's */
    }
}

} // namespace

hipError_t launch_ts_demux(const TsArgs& a, hipStream_t st)
{
    const uint32_t blocks = (uint32_t)((a.packets + kTsPacketsPerBlock - 1) / kTsPacketsPerBlock);
    const hipError_t e = begin_launches(a.ev_begin, st);
    if (e != hipSuccess) return e;
    if (blocks) hipLaunchKernelGGL(k_ts_count, dim3(blocks), dim3(kTT), 0, st, a);
    hipLaunchKernelGGL(k_ts_scan, dim3(1), dim3(kTT), 0, st, a, blocks);
    if (a.out && blocks) {
        if (a.pes) hipLaunchKernelGGL(k_ts_place, dim3(blocks), dim3(kTT), 0, st, a);
        hipLaunchKernelGGL(k_ts_copy, dim3(blocks), dim3(kTT), 0, st, a);
    }
    return end_launches(a.ev_end, st);
}

} // namespace hbs

extern "C" {

int hbs_ts_packet_host(const uint8_t* packet, int packet_bytes, int pid, hbs_ts_packet* out)
{
    return hbs::ts_packet_host(packet, packet_bytes, pid, out);
}

int hbs_ts_find_pid_host(const uint8_t* bytes, uint64_t n, int packet_bytes, int stream_type, int* program_out)
{
    return hbs::ts_find_pid_host(bytes, n, packet_bytes, stream_type, program_out);
}

}
