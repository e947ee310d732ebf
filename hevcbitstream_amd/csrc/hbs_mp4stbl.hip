/*
 * hbs_mp4stbl.hip -- hbs_mp4_stbl_samples: the sample table boxes (stsz, stco / co64, stsc, stts, ctts, stss) of a progressive
 * MP4 in device memory -> per sample its offset, size, decode time, presentation time and flags (include/hevcbitstream_amd.h;
 * the boxes' rules are stbl_heads, stbl_stsc_entry, stbl_stss_entry, stbl_join and stbl_place, hbs_mp4stbl.h).  Two "count,
 * scan, place" plans, one over the tables' entries, one over the samples; no launch waits for another workgroup, every grid
 * is sized by the payloads' byte counts or by sample_cap, none by a count read from a box:
 *
 *   k_st_head      one lane: the six fixed parts, versions and lengths; the counts N, C, E, T, K, S into the control words
 *   k_st_runs<0>   a lane an entry index, of all four run tables at once: the stsc entry against its neighbours and its
 *                  samples (stbl_run_samples), the stts entry's count and count x delta as two 32-bit halves, the ctts entry's
 *                  count, the stss number against the one in front; per workgroup the five sums and 1 + the first broken box
 *   k_st_scan      one workgroup: exclusive scan of those (scan_parts); the coverage rules of stsc and stts; the table error;
 *                  whether N fits sample_cap
 *   k_st_sizes     PLAN ONLY, a lane a size of a stsz that is a table: per workgroup the sample bytes.  A stsz of constant size
 *                  is settled in closed form by k_st_finish, whatever its count
 *   k_st_runs<1>   WITH OUTPUTS, the entries once more, with the sums in front: the first sample of every stsc, stts and ctts
 *                  entry and the time at which every stts entry begins
 *   k_st_samp<0>   THE HOT PATH, a lane a sample: its stsc run by a search among the runs' first samples (seek: two searches a
 *                  workgroup for its first and last sample, then a search a lane between the two), its chunk and place in it
 *                  by one 32-bit division; a segmented sum of the sizes over the workgroup that restarts at every chunk
 *                  (block_seg_excl); per workgroup the sum of its last chunk and whether a chunk began in it
 *   k_st_scan_samp one workgroup: the segmented scan of those over the workgroups (seg_scan_parts)
 *   k_st_samp<1>   the samples once more, with what their chunks bring along, and their stts and ctts entries found the same
 *                  way: offset, dts and pts of every sample checked (stbl_place); per workgroup the bytes and 1 + its lowest bad
 *                  sample
 *   k_st_finish    one workgroup: the totals, the error, the summary
 *   k_st_samp<2>   the samples a third time: the five tables; the sync bit by a search among the stss numbers
 *
 * Traffic: the run tables twice (three times their head and tail entries), with outputs 32 bytes of scratch an entry; the sizes
 * and chunk offsets three times.  No mdat byte is read.
 */
#include <hip/hip_runtime.h>
#include "hbs_mp4stbl.h"
#include "hbs_plan.h"

namespace hbs {
namespace {

constexpr int kST = kStLanes;
static_assert(kStLanes == kPlanLanes, "the plan's workgroups share block_scan's instances with scan_parts");

enum : int { kErr = 0, kN = 1, kC = 2, kE = 3, kT = 4, kK = 5, kS = 6, kSsz = 7, kCttsV = 8, kBadBox = 9, kStop = 10 };   /* ctl words */
/* kStop: 1 a table error, 2 N > sample_cap */

__global__ __launch_bounds__(64) void k_st_head(StblArgs a)
{
    if (threadIdx.x != 0) return;
    StblHead h;
    stbl_heads(a.src, a.box, a.co64, h);
    a.ctl[kErr] = 0; a.ctl[kN] = h.N; a.ctl[kC] = h.C; a.ctl[kE] = h.E; a.ctl[kT] = h.T; a.ctl[kK] = h.K; a.ctl[kS] = h.S;
    a.ctl[kSsz] = h.ssz; a.ctl[kCttsV] = h.ctts_v; a.ctl[kBadBox] = h.bad; a.ctl[kStop] = 0;
}

/* ---- entries ----------------------------------------------------------------------------------------------------------- */

template <int PLACE>
__global__ __launch_bounds__(kST) void k_st_runs(StblArgs a)
{
    if (PLACE && a.ctl[kStop] != 0) return;
    const uint64_t i = (uint64_t)blockIdx.x * kST + threadIdx.x;
    const uint64_t C = a.ctl[kC], E = a.ctl[kE], T = a.ctl[kT], K = a.ctl[kK], S = a.ctl[kS];
    uint64_t v[5] = {0, 0, 0, 0, 0}, bad = 0;
    if (i < E) {
        uint32_t fc, spc;
        uint64_t chunks;
        if (stbl_stsc_entry(a.src, a.box[kStsc].off + 8u, i, E, C, fc, spc, chunks)) v[0] = stbl_run_samples(chunks, spc);
        else bad = 1u + kStsc;
    }
    if (i < T) {
        const uint64_t at = a.box[kStts].off + 8u + i * 8u;
        const uint64_t cnt = rd_be32(a.src, at), prod = cnt * rd_be32(a.src, at + 4u);
        v[1] = cnt; v[2] = prod >> 32; v[3] = prod & 0xFFFFFFFFull;
    }
    if (i < K) v[4] = rd_be32(a.src, a.box[kCtts].off + 8u + i * 8u);
    if (!PLACE && i < S) {
        uint32_t number;
        if (!stbl_stss_entry(a.src, a.box[kStss].off + 8u, i, number) && !bad) bad = 1u + kStss;
    }
    unsigned long long* part = a.part_r + (uint64_t)blockIdx.x * 8;
    uint64_t ex[5], tot[5];
    if (!PLACE) {
        bad = block_min_nonzero(bad);
        block_scan<5, kST>(v, ex, tot);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int q = 0; q < 5; ++q) part[q] = tot[q];
            part[5] = bad;
        }
        return;
    }
    block_scan<5, kST>(v, ex, tot);
    if (i < E) a.stsc_first[i] = part[0] + ex[0];
    if (i < T) { a.stts_first[i] = part[1] + ex[1]; a.stts_time[i] = stbl_join(part[2] + ex[2], part[3] + ex[3]); }
    if (i < K) a.ctts_first[i] = part[4] + ex[4];
}

__global__ __launch_bounds__(kPlanLanes) void k_st_scan(StblArgs a, uint64_t entry_blocks)
{
    uint64_t carry[5];
    const uint64_t flag = scan_parts<5>(a.part_r, entry_blocks, carry);
    if (threadIdx.x == 0) {
        const uint64_t N = a.ctl[kN];
        uint64_t bad = a.ctl[kBadBox];
        if (flag && (!bad || flag < bad)) bad = flag;
        /* the coverage rules: the chunks hold N samples or more, the stts counts sum to N or more */
        if (carry[0] < N && (!bad || 1u + kStsc < bad)) bad = 1u + kStsc;
        if (carry[1] < N && (!bad || 1u + kStts < bad)) bad = 1u + kStts;
        a.ctl[kBadBox] = bad;
        a.ctl[kStop] = bad ? 1 : (a.out && N > a.sample_cap) ? 2 : 0;
    }
}

/* PLAN ONLY: the bytes of the samples of a stsz that is a table */
__global__ __launch_bounds__(kST) void k_st_sizes(StblArgs a)
{
    if (a.ctl[kStop] != 0) return;
    const uint64_t k = (uint64_t)blockIdx.x * kST + threadIdx.x;
    uint64_t v = 0, ex, tot;
    if (k < a.ctl[kN] && a.ctl[kSsz] == 0) v = rd_be32(a.src, a.box[kStsz].off + 12u + k * 4u);
    block_scan<1, kST>(&v, &ex, &tot);
    if (threadIdx.x == 0) { a.part_c[(uint64_t)blockIdx.x * 8] = tot; a.part_c[(uint64_t)blockIdx.x * 8 + 1] = 0; }
}

/* ---- samples ----------------------------------------------------------------------------------------------------------- */

/* the last entry in [lo, hi] whose first sample is k or in front of it (first[lo] <= k; first does not decrease) */
__device__ __forceinline__ uint64_t seek_in(const unsigned long long* first, uint64_t lo, uint64_t hi, uint64_t k)
{
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo + 1) / 2;
        if (first[mid] <= k) lo = mid; else hi = mid - 1;
    }
    return lo;
}

/* The run (of `count` >= 1, first[0] == 0) that holds sample k of a workgroup whose samples are [k0, k1]: every lane searches
 * the whole table for k0 and then for k1 -- the same words in all lanes, log2(count) steps -- and its own k only between the
 * two.  A table of one entry costs no step; in a table of an entry a sample the lane's own search has 8 steps within 2 KiB
 * that the workgroup shares.  (Entries of count 0 make the window longer than the workgroup, never wrong.) */
__device__ __forceinline__ uint64_t seek(const unsigned long long* first, uint64_t count, uint64_t k0, uint64_t k1, uint64_t k)
{
    const uint64_t lo = seek_in(first, 0, count - 1, k0);
    const uint64_t hi = seek_in(first, lo, count - 1, k1);
    return seek_in(first, lo, hi, k);
}

/* whether sample number k + 1 is among the S strictly increasing stss numbers: a search of the whole table for the workgroup's
 * first number, then at most kST numbers can lie in its range */
__device__ __forceinline__ bool stss_has(const uint8_t* p, uint64_t entries, uint64_t S, uint64_t k0, uint64_t k)
{
    uint64_t lo = 0, hi = S;                                   /* the first index whose number is k0 + 1 or more */
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if ((uint64_t)rd_be32(p, entries + mid * 4u) < k0 + 1u) lo = mid + 1; else hi = mid;
    }
    hi = lo + kST < S ? lo + kST : S;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if ((uint64_t)rd_be32(p, entries + mid * 4u) < k + 1u) lo = mid + 1; else hi = mid;
    }
    return lo < S && (uint64_t)rd_be32(p, entries + lo * 4u) == k + 1u;
}

/* MODE 0 count, 1 check, 2 place */
template <int MODE>
__global__ __launch_bounds__(kST) void k_st_samp(StblArgs a)
{
    if (a.ctl[MODE == 2 ? kErr : kStop] != 0) return;
    const uint64_t N = a.ctl[kN];
    const uint64_t k0 = (uint64_t)blockIdx.x * kST, k = k0 + threadIdx.x;
    const uint64_t k1 = k0 + kST - 1 < N ? k0 + kST - 1 : N - 1;
    const bool in = k < N;
    uint64_t v = 0, chunk_off = 0;
    bool head = false;
    if (in) {
        const uint32_t ssz = (uint32_t)a.ctl[kSsz];
        v = ssz ? ssz : rd_be32(a.src, a.box[kStsz].off + 12u + k * 4u);
        const uint64_t e = seek(a.stsc_first, a.ctl[kE], k0, k1, k);
        const uint64_t at = a.box[kStsc].off + 8u + e * 12u;
        const uint32_t fc = rd_be32(a.src, at), spc = rd_be32(a.src, at + 4u);
        const uint32_t r = (uint32_t)(k - a.stsc_first[e]);   /* (k < 2^32; the run holds sample k, so spc != 0) */
        const uint64_t chunk = (uint64_t)(fc - 1u) + r / spc;
        head = r % spc == 0u;
        if (MODE) chunk_off = a.co64 ? rd_be64(a.src, a.box[kStco].off + 8u + chunk * 8u) : (uint64_t)rd_be32(a.src, a.box[kStco].off + 8u + chunk * 4u);
    }
    uint64_t ex, tot;
    bool exf, totf;
    block_seg_excl<1, kST>(&v, &head, &ex, &exf, &tot, &totf);
    unsigned long long* part = a.part_k + (uint64_t)blockIdx.x * 8;
    if (MODE == 0) {
        if (threadIdx.x == 0) { part[0] = tot; part[1] = totf ? 1 : 0; }
        return;
    }
    const uint64_t before = head ? 0 : exf ? ex : ex + part[0];
    uint64_t off = 0, dts = 0, pts = 0;
    bool ok = true;
    if (in) {
        const uint64_t t = seek(a.stts_first, a.ctl[kT], k0, k1, k);
        const uint32_t delta = rd_be32(a.src, a.box[kStts].off + 8u + t * 8u + 4u);
        int64_t cts = 0;
        const uint64_t K = a.ctl[kK];
        if (K) {
            const uint64_t c = seek(a.ctts_first, K, k0, k1, k);
            const uint64_t at = a.box[kCtts].off + 8u + c * 8u;
            if (k - a.ctts_first[c] < (uint64_t)rd_be32(a.src, at)) cts = stbl_cts(rd_be32(a.src, at + 4u), (uint32_t)a.ctl[kCttsV]);
        }
        ok = stbl_place(chunk_off, before, (uint32_t)v, a.file_bytes, a.stts_time[t], k - a.stts_first[t], delta, cts, off, dts, pts);
    }
    if (MODE == 1) {
        const uint64_t bad = block_min_nonzero(ok ? 0 : k + 1);
        uint64_t bex, btot;
        block_scan<1, kST>(&v, &bex, &btot);
        if (threadIdx.x == 0) { a.part_c[(uint64_t)blockIdx.x * 8] = btot; a.part_c[(uint64_t)blockIdx.x * 8 + 1] = bad; }
        return;
    }
    if (!in) return;
    a.sample_off[k] = off; a.sample_size[k] = v;
    if (a.dts) a.dts[k] = dts;
    if (a.pts) a.pts[k] = pts;
    if (a.sample_flags) {
        const bool sync = a.box[kStss].bytes == 0 || stss_has(a.src, a.box[kStss].off + 8u, a.ctl[kS], k0, k);
        a.sample_flags[k] = sync ? 0u : 0x00010000u;
    }
}

__global__ __launch_bounds__(kPlanLanes) void k_st_scan_samp(StblArgs a, uint64_t samp_blocks)
{
    if (a.ctl[kStop] != 0) return;
    seg_scan_parts<1>(a.part_k, samp_blocks);
}

__global__ __launch_bounds__(kPlanLanes) void k_st_finish(StblArgs a, uint64_t blocks)
{
    const uint64_t stop = a.ctl[kStop];
    uint64_t carry[1] = {0}, bad_sample = 0;
    if (!stop) bad_sample = scan_parts<1>(a.part_c, blocks, carry);
    if (threadIdx.x == 0) {
        const uint64_t N = a.ctl[kN], ssz = a.ctl[kSsz];
        hbs_summary s;
        s.nal_count = 0; s.nal_found = 0; s.rbsp_bytes = 0; s.stream_bytes = a.n; s.stop_reason = 0;
        s.reserved[0] = 0; s.reserved[1] = 0; s.reserved[2] = 0;
        int32_t err = 0;
        if (stop == 1) { err = HBS_E_ARG; s.reserved[0] = a.ctl[kBadBox]; }
        else {
            s.nal_count = N; s.nal_found = a.ctl[kC];
            if (stop) err = HBS_E_CAPACITY;                            /* (N > sample_cap: the samples were not looked at) */
            else if (bad_sample) { err = HBS_E_ARG; s.reserved[2] = bad_sample; }
            else s.rbsp_bytes = (!a.out && ssz) ? N * ssz : carry[0];  /* (both factors below 2^32) */
        }
        s.error = err;
        a.ctl[kErr] = err ? 1 : 0;
        *a.summary = s;
    }
}

} // namespace

hipError_t launch_mp4_stbl_samples(const StblArgs& a, hipStream_t st)
{
    const uint64_t eb = stbl_entry_blocks(a), kb = a.out ? (a.sample_cap + kST - 1) / kST : 0, zb = a.out ? 0 : (a.cap[kStsz] + kST - 1) / kST;
    const hipError_t e = begin_launches(a.ev_begin, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_st_head, dim3(1), dim3(64), 0, st, a);
    if (eb) hipLaunchKernelGGL(k_st_runs<0>, dim3((unsigned)eb), dim3(kST), 0, st, a);
    hipLaunchKernelGGL(k_st_scan, dim3(1), dim3(kPlanLanes), 0, st, a, eb);
    if (!a.out && zb) hipLaunchKernelGGL(k_st_sizes, dim3((unsigned)zb), dim3(kST), 0, st, a);
    if (a.out && kb) {
        if (eb) hipLaunchKernelGGL(k_st_runs<1>, dim3((unsigned)eb), dim3(kST), 0, st, a);
        hipLaunchKernelGGL(k_st_samp<0>, dim3((unsigned)kb), dim3(kST), 0, st, a);
        hipLaunchKernelGGL(k_st_scan_samp, dim3(1), dim3(kPlanLanes), 0, st, a, kb);
        hipLaunchKernelGGL(k_st_samp<1>, dim3((unsigned)kb), dim3(kST), 0, st, a);
    }
    hipLaunchKernelGGL(k_st_finish, dim3(1), dim3(kPlanLanes), 0, st, a, a.out ? kb : zb);
    if (a.out && kb) hipLaunchKernelGGL(k_st_samp<2>, dim3((unsigned)kb), dim3(kST), 0, st, a);
    return end_launches(a.ev_end, st);
}

} // namespace hbs

extern "C" {

int hbs_mp4_stbl_find_host(const uint8_t* seg, uint64_t n, uint64_t base, uint32_t track_id, hbs_mp4_stbl* out)
{
    return hbs::mp4_stbl_find_host(seg, n, base, track_id, out);
}

int64_t hbs_mp4_track_read_host(const uint8_t* seg, uint64_t n, uint32_t track_id, hbs_mp4_track* out, uint64_t* nal_off, uint64_t* nal_bytes,
                                uint64_t cap)
{
    return hbs::mp4_track_read_host(seg, n, track_id, out, nal_off, nal_bytes, cap);
}

}
