/*
 * hbs_rtpord.hip -- hbs_rtp_order: a table of RTP packets in arrival order -> the table of the same packets by sequence number,
 * each once (include/hevcbitstream_amd.h is the specification; the rule is rtpo_read / rtpo_first_ext / rtpo_step / rtpo_late /
 * rtpo_span, hbs_rtpord.h).  A lane a packet or a lane a slot, 256 a workgroup; a slot is one extended sequence number of the
 * span.  No launch waits for another workgroup, and no packet byte but the headers is read:
 *
 *   k_rtpo_class   checks the table entry, then the packet's header (its first 16 bytes from one or two aligned 16-byte loads,
 *                  hbs_rtpbytes.h); leaves seq and "accepted" a packet, and per workgroup the accepted packets, the last
 *                  accepted packet with its seq, and 1 + its lowest faulty entry
 *   k_rtpo_scan_a  one workgroup: the last accepted packet in front of each workgroup (max_scan_parts, hbs_plan.h); on a fault
 *                  the error and the summary, and every later launch returns at once
 *   k_rtpo_diff    every accepted packet finds the accepted packet in front of it (the max-scan inside the workgroup and the
 *                  one over the workgroups) and forms sext16(seq - its seq), the first accepted packet its whole ext; the sums
 *                  inside the workgroup, and per workgroup their total
 *   k_rtpo_scan_d  one workgroup: the totals become what lies in front of each workgroup (scan_parts)
 *   k_rtpo_late    ext = the two sums; marks what is not late; per workgroup the highest and the lowest such ext and their number
 *   k_rtpo_scan_m  one workgroup: the highest ext in front of each workgroup; the lowest and the highest of all, their number,
 *                  base and span; HBS_E_CAPACITY when the span exceeds max_span
 *   k_rtpo_clear   `span` slots become empty
 *   k_rtpo_mark    every packet that is not late: atomicMin(slot[ext - base], its position) -- the first arrival owns the slot
 *   k_rtpo_moved   a packet that owns its slot is kept; it has moved when the running maximum in front of it is higher than its
 *                  ext; per workgroup their number
 *   k_rtpo_count   per 256 slots the taken ones
 *   k_rtpo_scan_s  one workgroup: the taken slots in front of each 256; kept, lost, duplicates, moved, the capacity, the summary.
 *                  A plan-only call ends here
 *   k_rtpo_place   a taken slot writes its owner's output row
 *
 * The launches over the slots have a grid sized by max_span (and capped); their workgroups loop up to the span k_rtpo_scan_m
 * found, so the work follows the span.  The only atomics are those on the slots: sums, minima and maxima over the workgroups
 * go through per-workgroup words that one workgroup reduces (tens of thousands of workgroups adding to one control word took
 * longer than all the rest of the call).  Traffic: per packet 16 B of the table and its header granule once, 12 B of scratch
 * written and read two to four times, an atomic; per slot 4 B written and read twice; per kept packet 16 B of the table once
 * more and 16 to 28 B of output.
 */
#include <hip/hip_runtime.h>
#include "hbs_rtpord.h"
#include "hbs_plan.h"
#include "hbs_rtpbytes.h"

namespace hbs {
namespace {

constexpr int kT = kPlanLanes;
static_assert(kRtpoLanes == kT, "one packet, or one slot, a lane");

enum : uint32_t { kRecAccepted = 1u << 16, kRecLive = 1u << 17 };
enum : int { kCtlError = 0, kCtlAccepted = 1, kCtlHighest = 2, kCtlLive = 3, kCtlBase = 4, kCtlSpan = 5 };

/* (1 + position) << 16 | seq of an accepted packet: the later packet has the higher key */
__device__ __forceinline__ uint64_t accepted_key(uint64_t p, uint32_t seq) { return ((p + 1u) << 16) | seq; }

__device__ __forceinline__ void write_summary(const RtpoArgs& a, int32_t err, uint64_t bad, uint64_t kept, uint64_t accepted, uint64_t span,
                                              uint64_t highest, uint64_t lost, uint64_t dup_moved)
{
    hbs_summary s;
    s.nal_count = kept; s.nal_found = accepted; s.rbsp_bytes = highest; s.stream_bytes = span;
    s.stop_reason = 0; s.error = err;
    s.reserved[0] = bad; s.reserved[1] = lost; s.reserved[2] = dup_moved;
    *a.summary = s;
}

__global__ __launch_bounds__(kT) void k_rtpo_class(RtpoArgs a)
{
    const uint64_t p = (uint64_t)blockIdx.x * kT + threadIdx.x;
    uint64_t v[1] = {0};
    uint64_t bad = 0, key = 0;
    if (p < a.n_packets) {
        const uint64_t off = a.pkt_off[p], size = a.pkt_size[p];
        RtpoPacket x;
        x.cls = kRtpoFault; x.seq = 0;
        if (!(size > a.n || off > a.n - size || size < kRtpHeader)) x = rtpo_read(load_packet(a.src, off, size), size, a.q);
        if (x.cls == kRtpoFault) bad = p + 1;
        if (x.cls == kRtpoAccepted) { v[0] = 1; key = accepted_key(p, x.seq); }
        a.rec[p] = x.seq | (x.cls == kRtpoAccepted ? kRecAccepted : 0u);
    }
    bad = block_min_nonzero(bad);
    uint64_t ex[1], tot[1];
    block_scan<1, kT>(v, ex, tot);
    uint64_t before, last;
    block_excl_max<uint64_t, 1, kT>(&key, &before, &last);
    if (threadIdx.x == 0) {
        unsigned long long* q = a.part_a + (uint64_t)blockIdx.x * 8;
        q[0] = tot[0]; q[1] = bad;
        a.last_a[blockIdx.x] = last;
    }
}

__global__ __launch_bounds__(kT) void k_rtpo_scan_a(RtpoArgs a, uint64_t blocks)
{
    uint64_t carry[1];
    const uint64_t bad = scan_parts<1>(a.part_a, blocks, carry);
    (void)max_scan_parts(a.last_a, blocks);
    if (threadIdx.x != 0) return;
    a.ctl[kCtlError] = bad ? (unsigned long long)(uint32_t)HBS_E_ARG : 0ull;
    a.ctl[kCtlAccepted] = carry[0];
    for (int i = kCtlHighest; i <= kCtlSpan; ++i) a.ctl[i] = 0;
    if (bad) write_summary(a, HBS_E_ARG, bad, 0, 0, 0, 0, 0, 0);
}

__global__ __launch_bounds__(kT) void k_rtpo_diff(RtpoArgs a)
{
    if (a.ctl[kCtlError] != 0) return;
    const uint64_t p = (uint64_t)blockIdx.x * kT + threadIdx.x;
    const uint32_t rec = p < a.n_packets ? a.rec[p] : 0u;
    const bool acc = (rec & kRecAccepted) != 0;
    const uint32_t seq = rec & 0xFFFFu;
    const uint64_t key = acc ? accepted_key(p, seq) : 0;
    uint64_t before, all;
    block_excl_max<uint64_t, 1, kT>(&key, &before, &all);
    uint64_t v[1] = {0};
    if (acc) {
        const uint64_t far = a.last_a[blockIdx.x];
        if (far > before) before = far;
        v[0] = before ? rtpo_step((uint32_t)(before & 0xFFFFu), seq) : rtpo_first_ext(a.q, seq);
    }
    uint64_t ex[1], tot[1];
    block_scan<1, kT>(v, ex, tot);
    if (acc) a.ext[p] = ex[0] + v[0];
    if (threadIdx.x == 0) {
        unsigned long long* q = a.part_d + (uint64_t)blockIdx.x * 8;
        q[0] = tot[0]; q[1] = 0;
    }
}

__global__ __launch_bounds__(kT) void k_rtpo_scan_d(RtpoArgs a, uint64_t blocks)
{
    if (a.ctl[kCtlError] != 0) return;
    uint64_t carry[1];
    (void)scan_parts<1>(a.part_d, blocks, carry);
}

__global__ __launch_bounds__(kT) void k_rtpo_late(RtpoArgs a)
{
    if (a.ctl[kCtlError] != 0) return;
    const uint64_t p = (uint64_t)blockIdx.x * kT + threadIdx.x;
    const uint32_t rec = p < a.n_packets ? a.rec[p] : 0u;
    const bool acc = (rec & kRecAccepted) != 0;
    uint64_t ext = 0;
    bool live = false;
    if (acc) {
        ext = a.ext[p] + a.part_d[(uint64_t)blockIdx.x * 8];
        a.ext[p] = ext;
        live = !rtpo_late(a.q, ext);
        if (live) a.rec[p] = rec | kRecLive;
    }
    const uint64_t v[2] = {live ? ext : 0, live ? ~ext : 0};       /* (ext is above 2^47: neither is 0 for a packet that counts) */
    uint64_t ex[2], tot[2];
    block_excl_max<uint64_t, 2, kT>(v, ex, tot);
    const int count = __syncthreads_count(live ? 1 : 0);
    if (threadIdx.x == 0) {
        a.last_m[blockIdx.x] = tot[0];
        a.low_m[2 * (uint64_t)blockIdx.x] = tot[1]; a.low_m[2 * (uint64_t)blockIdx.x + 1] = (unsigned long long)count;
    }
}

/* the sum of x over the workgroup's lanes */
__device__ __forceinline__ uint64_t block_sum(uint64_t x)
{
    uint64_t v[1] = {x}, ex[1], tot[1];
    block_scan<1, kT>(v, ex, tot);
    return tot[0];
}

__global__ __launch_bounds__(kT) void k_rtpo_scan_m(RtpoArgs a, uint64_t blocks)
{
    if (a.ctl[kCtlError] != 0) return;
    const uint64_t highest = max_scan_parts(a.last_m, blocks);
    uint64_t not_lowest = 0, count = 0;
    for (uint64_t i = threadIdx.x; i < blocks; i += kT) {
        const uint64_t x = a.low_m[2 * i];
        if (x > not_lowest) not_lowest = x;
        count += a.low_m[2 * i + 1];
    }
    uint64_t before, all;
    block_excl_max<uint64_t, 1, kT>(&not_lowest, &before, &all);
    const uint64_t live = block_sum(count), lowest = ~all;
    if (threadIdx.x != 0) return;
    const uint64_t span = rtpo_span(a.q, live, lowest, highest);
    a.ctl[kCtlHighest] = highest; a.ctl[kCtlLive] = live;
    a.ctl[kCtlBase] = rtpo_base(a.q, lowest);
    a.ctl[kCtlSpan] = span;
    if (span > a.q.max_span) {
        a.ctl[kCtlError] = (unsigned long long)(uint32_t)HBS_E_CAPACITY;
        write_summary(a, HBS_E_CAPACITY, 0, 0, a.ctl[kCtlAccepted], span, 0, 0, 0);
    }
}

__global__ __launch_bounds__(kT) void k_rtpo_clear(RtpoArgs a)
{
    if (a.ctl[kCtlError] != 0) return;
    const uint64_t quads = (a.ctl[kCtlSpan] + 3u) / 4u;              /* (the slots end on a multiple of 256 bytes) */
    u32x4 e;
    e.x = e.y = e.z = e.w = kRtpoEmpty;
    u32x4* const slot = reinterpret_cast<u32x4*>(a.slot);
    for (uint64_t i = (uint64_t)blockIdx.x * kT + threadIdx.x; i < quads; i += (uint64_t)gridDim.x * kT) slot[i] = e;
}

__global__ __launch_bounds__(kT) void k_rtpo_mark(RtpoArgs a)
{
    if (a.ctl[kCtlError] != 0) return;
    const uint64_t p = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (p >= a.n_packets || !(a.rec[p] & kRecLive)) return;
    atomicMin(a.slot + (a.ext[p] - a.ctl[kCtlBase]), (uint32_t)p);
}

__global__ __launch_bounds__(kT) void k_rtpo_moved(RtpoArgs a)
{
    if (a.ctl[kCtlError] != 0) return;
    const uint64_t p = (uint64_t)blockIdx.x * kT + threadIdx.x;
    const bool live = p < a.n_packets && (a.rec[p] & kRecLive);
    const uint64_t ext = live ? a.ext[p] : 0;
    uint64_t before, all;
    block_excl_max<uint64_t, 1, kT>(&ext, &before, &all);
    bool moved = false;
    if (live) {
        const uint64_t far = a.last_m[blockIdx.x];
        if (far > before) before = far;
        moved = before > ext && a.slot[ext - a.ctl[kCtlBase]] == (uint32_t)p;
    }
    const int count = __syncthreads_count(moved ? 1 : 0);
    if (threadIdx.x == 0) a.moved_m[blockIdx.x] = (unsigned long long)count;
}

__global__ __launch_bounds__(kT) void k_rtpo_count(RtpoArgs a)
{
    if (a.ctl[kCtlError] != 0) return;
    const uint64_t span = a.ctl[kCtlSpan], sblocks = rtpo_blocks(span);
    for (uint64_t b = blockIdx.x; b < sblocks; b += gridDim.x) {
        const uint64_t i = b * kT + threadIdx.x;
        const int count = __syncthreads_count(i < span && a.slot[i] != kRtpoEmpty ? 1 : 0);
        if (threadIdx.x == 0) { a.part_s[b * 8] = (unsigned long long)count; a.part_s[b * 8 + 1] = 0; }
    }
}

__global__ __launch_bounds__(kT) void k_rtpo_scan_s(RtpoArgs a, uint64_t blocks)
{
    if (a.ctl[kCtlError] != 0) return;
    const uint64_t span = a.ctl[kCtlSpan];
    uint64_t carry[1];
    (void)scan_parts<1>(a.part_s, rtpo_blocks(span), carry);
    uint64_t count = 0;
    for (uint64_t i = threadIdx.x; i < blocks; i += kT) count += a.moved_m[i];
    const uint64_t moved = block_sum(count);
    if (threadIdx.x != 0) return;
    const uint64_t kept = carry[0], live = a.ctl[kCtlLive];
    const int32_t err = a.off_out && kept > a.out_cap ? HBS_E_CAPACITY : 0;
    a.ctl[kCtlError] = (unsigned long long)(uint32_t)err;
    write_summary(a, err, 0, kept, a.ctl[kCtlAccepted], span, kept ? a.ctl[kCtlHighest] : 0, span - kept, ((live - kept) << 32) | moved);
}

__global__ __launch_bounds__(kT) void k_rtpo_place(RtpoArgs a)
{
    if (a.ctl[kCtlError] != 0) return;
    const uint64_t span = a.ctl[kCtlSpan], base = a.ctl[kCtlBase], sblocks = rtpo_blocks(span);
    for (uint64_t b = blockIdx.x; b < sblocks; b += gridDim.x) {
        const uint64_t i = b * kT + threadIdx.x;
        const uint32_t p = i < span ? a.slot[i] : kRtpoEmpty;
        uint64_t v[1] = {p != kRtpoEmpty ? 1u : 0u};
        uint64_t ex[1], tot[1];
        block_scan<1, kT>(v, ex, tot);
        if (p == kRtpoEmpty) continue;
        const uint64_t k = a.part_s[b * 8] + ex[0];
        a.off_out[k] = a.pkt_off[p]; a.size_out[k] = a.pkt_size[p];
        if (a.src_out) a.src_out[k] = p;
        if (a.ext_out) a.ext_out[k] = base + i;
    }
}

} // namespace

hipError_t launch_rtp_order(const RtpoArgs& a, hipStream_t st)
{
    const uint64_t blocks = rtpo_blocks(a.n_packets);
    const dim3 grid((unsigned)blocks), sgrid((unsigned)a.slot_grid), lanes(kT);
    const hipError_t e = begin_launches(a.ev_begin, st);
    if (e != hipSuccess) return e;
    if (blocks) hipLaunchKernelGGL(k_rtpo_class, grid, lanes, 0, st, a);
    hipLaunchKernelGGL(k_rtpo_scan_a, dim3(1), lanes, 0, st, a, blocks);
    if (blocks) hipLaunchKernelGGL(k_rtpo_diff, grid, lanes, 0, st, a);
    hipLaunchKernelGGL(k_rtpo_scan_d, dim3(1), lanes, 0, st, a, blocks);
    if (blocks) hipLaunchKernelGGL(k_rtpo_late, grid, lanes, 0, st, a);
    hipLaunchKernelGGL(k_rtpo_scan_m, dim3(1), lanes, 0, st, a, blocks);
    if (blocks) {
        hipLaunchKernelGGL(k_rtpo_clear, sgrid, lanes, 0, st, a);
        hipLaunchKernelGGL(k_rtpo_mark, grid, lanes, 0, st, a);
        hipLaunchKernelGGL(k_rtpo_moved, grid, lanes, 0, st, a);
        hipLaunchKernelGGL(k_rtpo_count, sgrid, lanes, 0, st, a);
    }
    hipLaunchKernelGGL(k_rtpo_scan_s, dim3(1), lanes, 0, st, a, blocks);
    if (a.off_out && blocks) hipLaunchKernelGGL(k_rtpo_place, sgrid, lanes, 0, st, a);
    return end_launches(a.ev_end, st);
}

} // namespace hbs
