/*
 * hbs_mp4stblw.hip -- hbs_mp4_stbl_write: per sample its offset, size, decode time, presentation time and flags -> the sample
 * table boxes stts, ctts, stss, stsc, stsz, stco / co64 of a progressive MP4, as whole boxes one behind the other
 * (include/hevcbitstream_amd.h; the rules are stblw_lane, stblw_chunk_start, stblw_run_start, stblw_stsz_constant and
 * stblw_layout, hbs_mp4stblw.h) -- and hbs_mp4_moov_host.  Two "count, scan, place" plans, one over the samples, one over the
 * chunks and runs they make; no launch waits for another workgroup, every grid is sized by n_samples:
 *
 *   k_sw_breaks     only with max_chunk_samples: a lane a sample, per workgroup 1 + its last sample that is not contiguous
 *   k_sw_max        ... one workgroup: the maximum of the workgroups in front (max_scan_parts), so that every lane knows s(k)
 *   k_sw_samp<0>    a lane a sample (stblw_lane: its own row and its left neighbour's): whether a chunk, an stts run or a ctts
 *                   run begins, whether it is a sync sample, 1 + k if it breaks a rule; its size, delta, whether its size is
 *                   other than the first sample's, whether its cts is negative.  Per workgroup two times four sums and the
 *                   lowest bad sample
 *   k_sw_plan       one workgroup: the exclusive scans of those (scan_parts); C, the stts, ctts and stss counts, the sums; a
 *                   sample error ends the call here
 *   k_sw_samp<1>    the samples once more, with the sums in front: the first samples of the chunks and of the stts and ctts
 *                   runs, compacted into scratch
 *   k_sw_chunk<0>   a lane a chunk: its length from neighbouring first samples, whether an stsc entry begins; per workgroup
 *                   how many do
 *   k_sw_finish     one workgroup: the scan of those; the box sizes and offsets (stblw_layout), the box size error, capacity;
 *                   the summary, d_tables and the six box headers
 *   k_sw_chunk<1>   a lane a chunk and a run: the stco / co64 and stsc entries, the stts and ctts entries
 *   k_sw_fill       a lane a sample: the sizes of an stsz that is a table, the stss numbers
 *
 * Every store into d_out is one 32-bit word, byte-swapped once, at a 4-aligned offset; lanes of a workgroup store neighbouring
 * words.  Traffic: the sample tables three times (four with max_chunk_samples), 24 bytes of scratch a chunk or run at most.
 */
#include <hip/hip_runtime.h>
#include "hbs_mp4stblw.h"
#include "hbs_plan.h"

namespace hbs {
namespace {

constexpr int kSW = kSwLanes;
static_assert(kSwLanes == kPlanLanes, "the plan's workgroups share block_scan's instances with scan_parts");

/* ctl words */
enum : int { kStop = 0,                                     /* 0, 1 a sample error, 2 a box too large, 3 capacity                       */
             kC = 1, kT = 2, kK = 3, kS = 4,                /* chunks, stts entries, ctts entries, sync samples                         */
             kBytes = 5, kDur = 6, kDiffer = 7, kNeg = 8,   /* sums: sizes, deltas, sizes other than the first, negative cts            */
             kBad = 9, kConst = 10, kOff = 11 };            /* 1 + the lowest bad sample; the short stsz; kOff + b: box b's offset      */

__device__ __forceinline__ void put32(uint8_t* out, uint64_t at, uint32_t v)
{
    *reinterpret_cast<uint32_t*>(out + at) = __builtin_bswap32(v);
}

__device__ __forceinline__ bool breaks(const StblwIn& in, uint64_t k)
{
    return k == 0 || !stblw_contiguous(in.off[k - 1u], in.size[k - 1u], in.off[k]);
}

__global__ __launch_bounds__(kSW) void k_sw_breaks(StblwArgs a)
{
    const uint64_t k = (uint64_t)blockIdx.x * kSW + threadIdx.x;
    uint64_t v = k < a.in.n && breaks(a.in, k) ? k + 1u : 0u, ex, tot;
    block_excl_max<uint64_t, 1, kSW>(&v, &ex, &tot);
    if (threadIdx.x == 0) a.last[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kPlanLanes) void k_sw_max(StblwArgs a, uint64_t blocks)
{
    (void)max_scan_parts(a.last, blocks);
}

/* MODE 0 count, 1 compact */
template <int MODE>
__global__ __launch_bounds__(kSW) void k_sw_samp(StblwArgs a)
{
    if (MODE && a.ctl[kStop] != 0) return;
    const uint64_t k = (uint64_t)blockIdx.x * kSW + threadIdx.x;
    const bool in = k < a.in.n;
    StblwLane l;
    l.z = 0; l.o = 0; l.delta = 0; l.cts = 0; l.bad = false; l.brk = false; l.stts_run = false; l.ctts_run = false; l.sync = false;
    if (in) stblw_lane(a.in, k, l);
    bool chunk = l.brk;
    if (a.max_chunk) {                                         /* (the same in every lane) */
        uint64_t v = l.brk ? k + 1u : 0u, ex, tot;
        block_excl_max<uint64_t, 1, kSW>(&v, &ex, &tot);
        uint64_t s1 = a.last[blockIdx.x];                      /* 1 + s(k): sample 0 is never contiguous, so it is 1 or more */
        if (ex > s1) s1 = ex;
        if (v > s1) s1 = v;
        chunk = in && stblw_chunk_start(k, s1 - 1u, a.max_chunk);
    }
    uint64_t v[4] = {chunk ? 1u : 0u, l.stts_run ? 1u : 0u, l.ctts_run ? 1u : 0u, l.sync ? 1u : 0u}, ex[4], tot[4];
    block_scan<4, kSW>(v, ex, tot);
    unsigned long long* part = a.part_r + (uint64_t)blockIdx.x * 8;
    if (MODE == 0) {
        const bool bad = in && (l.bad || (chunk && !stblw_chunk_off_ok(l.o, a.co64)));
        const uint64_t lowest = block_min_nonzero(bad ? k + 1u : 0u);
        uint64_t w[4] = {l.z, l.delta, in && l.z != a.in.size[0] ? 1u : 0u, l.cts < 0 ? 1u : 0u}, wex[4], wtot[4];
        block_scan<4, kSW>(w, wex, wtot);
        if (threadIdx.x == 0) {
            unsigned long long* sums = a.part_s + (uint64_t)blockIdx.x * 8;
#pragma unroll
            for (int q = 0; q < 4; ++q) { part[q] = tot[q]; sums[q] = wtot[q]; }
            part[4] = lowest; sums[4] = 0;
        }
        return;
    }
    if (chunk) a.chunk_first[part[0] + ex[0]] = k;
    if (l.stts_run) a.stts_first[part[1] + ex[1]] = k;
    if (l.ctts_run) a.ctts_first[part[2] + ex[2]] = k;
}

__global__ __launch_bounds__(kPlanLanes) void k_sw_plan(StblwArgs a, uint64_t blocks)
{
    uint64_t runs[4], sums[4];
    const uint64_t bad = scan_parts<4>(a.part_r, blocks, runs);
    (void)scan_parts<4>(a.part_s, blocks, sums);
    if (threadIdx.x == 0) {
        a.ctl[kC] = runs[0]; a.ctl[kT] = runs[1]; a.ctl[kK] = runs[2]; a.ctl[kS] = runs[3];
        a.ctl[kBytes] = sums[0]; a.ctl[kDur] = sums[1]; a.ctl[kDiffer] = sums[2]; a.ctl[kNeg] = sums[3];
        a.ctl[kBad] = bad;
        a.ctl[kStop] = bad ? 1 : 0;
    }
}

/* the samples of chunk c < C */
__device__ __forceinline__ uint64_t chunk_len(const StblwArgs& a, uint64_t c, uint64_t C)
{
    return (c + 1u < C ? a.chunk_first[c + 1u] : a.in.n) - a.chunk_first[c];
}

/* MODE 0 count the stsc entries, 1 write the entries of stco / co64, stsc, stts and ctts */
template <int MODE>
__global__ __launch_bounds__(kSW) void k_sw_chunk(StblwArgs a)
{
    if (a.ctl[kStop] != 0) return;
    const uint64_t i = (uint64_t)blockIdx.x * kSW + threadIdx.x;
    const uint64_t N = a.in.n, C = a.ctl[kC];
    uint64_t len = 0, run = 0, ex, tot;
    if (i < C) {
        len = chunk_len(a, i, C);
        run = stblw_run_start(i, len, i ? chunk_len(a, i - 1u, C) : 0u) ? 1u : 0u;
    }
    block_scan<1, kSW>(&run, &ex, &tot);
    unsigned long long* part = a.part_c + (uint64_t)blockIdx.x * 8;
    if (MODE == 0) {
        if (threadIdx.x == 0) { part[0] = tot; part[1] = 0; }
        return;
    }
    if (i < C) {
        const uint64_t o = a.in.off[a.chunk_first[i]] + a.in.data_offset, at = a.ctl[kOff + kSwStco] + 16u;
        if (a.co64) { put32(a.out, at + i * 8u, (uint32_t)(o >> 32)); put32(a.out, at + i * 8u + 4u, (uint32_t)o); }
        else put32(a.out, at + i * 4u, (uint32_t)o);
        if (run) {
            const uint64_t e = a.ctl[kOff + kSwStsc] + 16u + (part[0] + ex) * 12u;
            put32(a.out, e, (uint32_t)(i + 1u)); put32(a.out, e + 4u, (uint32_t)len); put32(a.out, e + 8u, 1u);
        }
    }
    const uint64_t T = a.ctl[kT], K = a.ctl[kK];
    if (i < T) {
        const uint64_t f = a.stts_first[i], e = a.ctl[kOff + kSwStts] + 16u + i * 8u;
        uint64_t t, delta;
        (void)stblw_times(a.in, f, t, delta);
        put32(a.out, e, (uint32_t)((i + 1u < T ? a.stts_first[i + 1u] : N) - f)); put32(a.out, e + 4u, (uint32_t)delta);
    }
    if (i < K) {
        const uint64_t f = a.ctts_first[i], e = a.ctl[kOff + kSwCtts] + 16u + i * 8u;
        uint64_t t, delta;
        int64_t cts;
        (void)stblw_times(a.in, f, t, delta);
        (void)stblw_cts(a.in.pts[f], t, cts);
        put32(a.out, e, (uint32_t)((i + 1u < K ? a.ctts_first[i + 1u] : N) - f)); put32(a.out, e + 4u, (uint32_t)(int32_t)cts);
    }
}

__global__ __launch_bounds__(kPlanLanes) void k_sw_finish(StblwArgs a, uint64_t blocks)
{
    uint64_t stop = a.ctl[kStop];
    uint64_t E[1] = {0};
    if (!stop) (void)scan_parts<1>(a.part_c, blocks, E);
    if (threadIdx.x != 0) return;
    const uint64_t N = a.in.n;
    hbs_summary s;
    s.error = 0; s.nal_count = N; s.nal_found = 0; s.rbsp_bytes = 0; s.stream_bytes = 0; s.stop_reason = 0;
    s.reserved[0] = 0; s.reserved[1] = 0; s.reserved[2] = 0;
    uint64_t off[kSwBoxes], bytes[kSwBoxes], total = 0;
    const uint64_t entries[kSwBoxes] = {a.ctl[kT], a.ctl[kK], a.ctl[kS], E[0], N, a.ctl[kC]};
    bool constant = false;
    if (stop) { s.error = HBS_E_ARG; s.reserved[2] = a.ctl[kBad]; }
    else {
        constant = stblw_stsz_constant(N, a.ctl[kDiffer], N ? a.in.size[0] : 0u);
        const uint32_t box = stblw_layout(entries, a.in.pts != nullptr, a.in.sflags != nullptr, constant, a.co64, off, bytes, total);
        if (box) { stop = 2; s.error = HBS_E_ARG; s.reserved[0] = box; }
        else {
            s.nal_found = a.ctl[kC]; s.rbsp_bytes = a.ctl[kBytes]; s.stream_bytes = total; s.reserved[1] = a.ctl[kDur];
            if (a.out && a.out_cap < total) { stop = 3; s.error = HBS_E_CAPACITY; }
        }
    }
    a.ctl[kStop] = stop;
    *a.summary = s;
    if (stop) return;
    a.ctl[kConst] = constant ? 1 : 0;
    for (int b = 0; b < kSwBoxes; ++b) a.ctl[kOff + b] = off[b];
    if (a.tables) {
        hbs_mp4_stbl t;
        hbs_mp4_box_ref* ref[kSwBoxes] = {&t.stts, &t.ctts, &t.stss, &t.stsc, &t.stsz, &t.stco};
        for (int b = 0; b < kSwBoxes; ++b) { ref[b]->off = bytes[b] ? off[b] + 8u : 0u; ref[b]->bytes = bytes[b] ? bytes[b] - 8u : 0u; }
        t.flags = a.co64 ? (uint32_t)HBS_MP4_STBL_CO64 : 0u; t.reserved0 = 0; t.file_bytes = 0; t.reserved[0] = 0; t.reserved[1] = 0;
        *a.tables = t;
    }
    if (!a.out) return;
    for (int b = 0; b < kSwBoxes; ++b) {
        if (!bytes[b]) continue;
        uint64_t at = off[b];
        put32(a.out, at, (uint32_t)bytes[b]); put32(a.out, at + 4u, stblw_fourcc(b, a.co64));
        put32(a.out, at + 8u, b == kSwCtts && a.ctl[kNeg] ? 0x01000000u : 0u);
        at += 12u;
        if (b == kSwStsz) { put32(a.out, at, constant ? (uint32_t)a.in.size[0] : 0u); at += 4u; }
        put32(a.out, at, (uint32_t)entries[b]);
    }
}

__global__ __launch_bounds__(kSW) void k_sw_fill(StblwArgs a)
{
    if (a.ctl[kStop] != 0) return;
    const uint64_t k = (uint64_t)blockIdx.x * kSW + threadIdx.x;
    const bool in = k < a.in.n;
    if (in && !a.ctl[kConst]) put32(a.out, a.ctl[kOff + kSwStsz] + 20u + k * 4u, (uint32_t)a.in.size[k]);
    if (!a.in.sflags) return;                                  /* (the same in every lane) */
    uint64_t v = in && stblw_sync(a.in.sflags[k]) ? 1u : 0u, ex, tot;
    block_scan<1, kSW>(&v, &ex, &tot);
    if (v) put32(a.out, a.ctl[kOff + kSwStss] + 16u + (a.part_r[(uint64_t)blockIdx.x * 8 + 3] + ex) * 4u, (uint32_t)(k + 1u));
}

} // namespace

hipError_t launch_mp4_stbl_write(const StblwArgs& a, hipStream_t st)
{
    const uint64_t kb = stblw_blocks(a.in.n);
    const hipError_t e = begin_launches(a.ev_begin, st);
    if (e != hipSuccess) return e;
    if (kb) {
        if (a.max_chunk) {
            hipLaunchKernelGGL(k_sw_breaks, dim3((unsigned)kb), dim3(kSW), 0, st, a);
            hipLaunchKernelGGL(k_sw_max, dim3(1), dim3(kPlanLanes), 0, st, a, kb);
        }
        hipLaunchKernelGGL(k_sw_samp<0>, dim3((unsigned)kb), dim3(kSW), 0, st, a);
    }
    hipLaunchKernelGGL(k_sw_plan, dim3(1), dim3(kPlanLanes), 0, st, a, kb);
    if (kb) {
        hipLaunchKernelGGL(k_sw_samp<1>, dim3((unsigned)kb), dim3(kSW), 0, st, a);
        hipLaunchKernelGGL(k_sw_chunk<0>, dim3((unsigned)kb), dim3(kSW), 0, st, a);
    }
    hipLaunchKernelGGL(k_sw_finish, dim3(1), dim3(kPlanLanes), 0, st, a, kb);
    if (kb && a.out) {
        hipLaunchKernelGGL(k_sw_chunk<1>, dim3((unsigned)kb), dim3(kSW), 0, st, a);
        hipLaunchKernelGGL(k_sw_fill, dim3((unsigned)kb), dim3(kSW), 0, st, a);
    }
    return end_launches(a.ev_end, st);
}

} // namespace hbs

extern "C" {

uint64_t hbs_mp4_stbl_write_bytes_host(uint64_t n_samples, int with_ctts, int with_stss, uint32_t flags)
{
    return hbs::mp4_stbl_write_bytes(n_samples, with_ctts, with_stss, flags);
}

int64_t hbs_mp4_moov_host(const hbs_mp4_init_params* p, int flags, const uint8_t* const* nal, const uint64_t* nal_bytes, uint64_t n,
                          uint64_t duration, uint64_t tables_bytes, uint8_t* out, uint64_t cap)
{
    return hbs::mp4_moov_host(p, flags, nal, nal_bytes, n, duration, tables_bytes, out, cap);
}

}
