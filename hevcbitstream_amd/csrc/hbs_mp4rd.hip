/*
 * hbs_mp4rd.hip -- hbs_mp4_samples: the moof boxes of fragmented-MP4 segments in device memory -> a sample table (offset, size,
 * decode time, presentation time, flags) and a fragment table (include/hevcbitstream_amd.h; the boxes' rules are mp4rd_box,
 * mp4rd_moof, mp4rd_sample and mp4rd_place, hbs_mp4rd.h).  Three "count, scan, place" plans, one over the segments, one over the
 * moofs, one over the samples; no launch waits for another workgroup, none reads an mdat payload byte:
 *
 *   k_rd_seg<0>    a lane a segment, 256 a workgroup: checks the segment's range, walks its chain of top-level boxes and
 *                  counts the moofs; per workgroup their sum and 1 + its lowest segment with a chain error
 *   k_rd_scan_seg  one workgroup: exclusive scan of those sums (scan_parts); the moof count M, the control words
 *   k_rd_seg<1>    the chains once more, now with the moof numbers: each moof's offset, size, segment and the distance to the
 *                  next moof of its segment (or to the segment's end)
 *   k_rd_moof<0>   a lane a moof: walks its children (mfhd, the traf of the track, tfhd, tfdt, the truns) and counts the truns
 *                  that have samples and the samples; per workgroup the sums and 1 + its lowest moof with a moof error
 *   k_rd_scan_moof one workgroup: exclusive scan of both; the trun count and the sample count N
 *   k_rd_moof<1>   the moofs once more, with the numbers: a 64-byte record a trun (where its entries lie, its flags, its data
 *                  begin or that of the trun it continues, the tfdt time, the defaults resolved through tfhd and trex) and the
 *                  fragment table's record
 *   k_rd_moof<2>   PLAN ONLY, in place of <1> and the four sample kernels: the moof's lane goes through its truns' entries
 *                  itself, since no sample_cap sizes a grid -- a step an entry that has bytes, so the work is bounded by the
 *                  moof's size; a trun whose entries have no bytes (every field a default; its count is bounded by nothing)
 *                  is settled in closed form (mp4rd_run_good); per workgroup the sample bytes and 1 + its lowest bad sample
 *   k_rd_samp<0>   THE HOT PATH, a lane a sample: binary search of its trun among the truns' first samples, its entry's words by
 *                  aligned loads and alignbyte, the defaults; two segmented sums over the workgroup (block_seg_excl): the sizes
 *                  restart at every trun that has a data_offset and at every traf, the durations at every moof; per workgroup
 *                  the sums of its last runs and whether a run began in it
 *   k_rd_scan_samp one workgroup: the segmented scan of those over the workgroups (seg_scan_parts)
 *   k_rd_samp<1>   the samples once more, with what their runs bring along: offset, dts and pts of every sample checked; per
 *                  workgroup the sample bytes and 1 + its lowest bad sample
 *   k_rd_finish    one workgroup: the totals, the error, the summary
 *   k_rd_samp<2>   the samples a third time: the five tables;  k_rd_frags  a lane a moof: d_frag
 *
 * Traffic: the box headers along the chains three times (segment, moof count, moof place), the trun entries three times; 8 bytes
 * a segment, 96 a moof and 68 a sample of scratch.
 */
#include <hip/hip_runtime.h>
#include "hbs_mp4rd.h"
#include "hbs_plan.h"

namespace hbs {
namespace {

constexpr int kRT = kRdLanes;
static_assert(kRdLanes == kPlanLanes, "the plan's workgroups share block_scan's instances with scan_parts");

enum : int { kErr = 0, kMoofs = 1, kSamples = 2, kTruns = 3, kBadSeg = 4, kBadMoof = 5, kStop = 6 };      /* ctl words */

/* segment s: false when it leaves the buffer */
__device__ __forceinline__ bool seg_range(const Mp4RdArgs& a, uint64_t s, uint64_t& off, uint64_t& size)
{
    if (!a.seg) { off = 0; size = a.n; return true; }
    const unsigned long long* r = reinterpret_cast<const unsigned long long*>(a.seg + s * a.seg_stride);
    off = r[0]; size = r[1];
    return off <= a.n && size <= a.n - off;
}

/* the chain of top-level boxes of d_in[off, off + size): on_moof(j, at, box) for its j-th moof; false: a chain error */
template <class F>
__device__ __forceinline__ bool walk_segment(const uint8_t* p, uint64_t off, uint64_t size, uint64_t& moofs, F&& on_moof)
{
    const uint64_t end = off + size;
    moofs = 0;
    for (uint64_t q = off; q < end;) {
        Mp4Box b;
        if (!mp4rd_box(p, q, end, b)) return false;
        if (b.type == HBS_MP4_FOURCC('m', 'o', 'o', 'f')) { on_moof(moofs, q, b); moofs += 1; }
        q += b.size;
    }
    return true;
}

template <int PLACE>
__global__ __launch_bounds__(kRT) void k_rd_seg(Mp4RdArgs a)
{
    if (PLACE && a.ctl[kStop] != 0) return;
    const uint64_t s = (uint64_t)blockIdx.x * kRT + threadIdx.x;
    const bool in = s < a.n_segs;
    uint64_t off = 0, size = 0;
    if (!PLACE) {
        uint64_t cnt = 0, bad = 0;
        if (in) {
            if (!seg_range(a, s, off, size) || !walk_segment(a.src, off, size, cnt, [](uint64_t, uint64_t, const Mp4Box&) {})) { bad = s + 1; cnt = 0; }
            a.seg_cnt[s] = cnt;
        }
        bad = block_min_nonzero(bad);
        uint64_t ex, tot;
        block_scan<1, kRT>(&cnt, &ex, &tot);
        if (threadIdx.x == 0) { a.part_s[(uint64_t)blockIdx.x * 8] = tot; a.part_s[(uint64_t)blockIdx.x * 8 + 1] = bad; }
        return;
    }
    const uint64_t cnt = in ? a.seg_cnt[s] : 0;
    uint64_t ex, tot;
    block_scan<1, kRT>(&cnt, &ex, &tot);
    if (!cnt) return;
    const uint64_t base = a.part_s[(uint64_t)blockIdx.x * 8] + ex;
    (void)seg_range(a, s, off, size);
    uint64_t n = 0, prev = 0;
    (void)walk_segment(a.src, off, size, n, [&](uint64_t j, uint64_t at, const Mp4Box& b) {
        a.moof_at[base + j] = at; a.moof_size[base + j] = b.size | (b.head == 16u ? kRdLarge : 0); a.moof_seg[base + j] = off;
        if (j) a.moof_span[base + j - 1] = at - prev;
        prev = at;
    });
    a.moof_span[base + n - 1] = off + size - prev;
}

__global__ __launch_bounds__(kPlanLanes) void k_rd_scan_seg(Mp4RdArgs a, uint64_t seg_blocks)
{
    uint64_t carry[1];
    const uint64_t bad = scan_parts<1>(a.part_s, seg_blocks, carry);
    if (threadIdx.x == 0) {
        a.ctl[kErr] = 0; a.ctl[kMoofs] = carry[0]; a.ctl[kSamples] = 0; a.ctl[kTruns] = 0; a.ctl[kBadSeg] = bad; a.ctl[kBadMoof] = 0;
        a.ctl[kStop] = (bad || carry[0] > a.moof_cap) ? 1 : 0;
    }
}

/* ---- moofs ------------------------------------------------------------------------------------------------------------- */

/* MODE 0 count, 1 place (trun records, the fragment's record), 2 plan only: the lane evaluates its samples itself */
template <int MODE>
__global__ __launch_bounds__(kRT) void k_rd_moof(Mp4RdArgs a)
{
    if (a.ctl[kStop] != 0) return;
    const uint64_t m = (uint64_t)blockIdx.x * kRT + threadIdx.x;
    const bool in = m < a.ctl[kMoofs];
    uint64_t at = 0, size = 0, seg = 0;
    uint32_t head = 8;
    if (in) { at = a.moof_at[m]; size = a.moof_size[m] & ~kRdLarge; head = (a.moof_size[m] & kRdLarge) ? 16u : 8u; seg = a.moof_seg[m]; }
    Mp4Moof mo;
    if (MODE == 0) {
        uint64_t v[2] = {0, 0}, bad = 0;
        if (in) {
            if (mp4rd_moof(a.src, seg, at, size, head, a.x, mo, [](uint64_t, const Mp4TrunRec&) {})) { v[0] = mo.truns; v[1] = mo.samples; }
            else bad = m + 1;
            a.moof_cnt[2 * m] = v[0]; a.moof_cnt[2 * m + 1] = v[1];
        }
        bad = block_min_nonzero(bad);
        uint64_t ex[2], tot[2];
        block_scan<2, kRT>(v, ex, tot);
        if (threadIdx.x == 0) {
            unsigned long long* p = a.part_m + (uint64_t)blockIdx.x * 8;
            p[0] = tot[0]; p[1] = tot[1]; p[2] = bad;
        }
        return;
    }
    uint64_t v[2] = {0, 0};
    if (in) { v[0] = a.moof_cnt[2 * m]; v[1] = a.moof_cnt[2 * m + 1]; }
    uint64_t ex[2], tot[2];
    block_scan<2, kRT>(v, ex, tot);
    const uint64_t t0 = a.part_m[(uint64_t)blockIdx.x * 8] + ex[0], k0 = a.part_m[(uint64_t)blockIdx.x * 8 + 1] + ex[1];
    uint32_t first_flags = 0x00010000u;
    uint64_t bytes = 0, bad = 0;
    if (in) {
        if (MODE == 1) {
            (void)mp4rd_moof(a.src, seg, at, size, head, a.x, mo, [&](uint64_t i, const Mp4TrunRec& r0) {
                Mp4TrunRec r = r0;
                if (i == 0) first_flags = mp4rd_sample(a.src, r, 0).flags;
                r.first = (uint32_t)(k0 + r0.first); r.moof = (uint32_t)m;
                a.trun[t0 + i] = r;
                a.trun_first[t0 + i] = r.first;
            });
        } else {
            uint64_t before = 0, dur_before = 0, k = k0;
            (void)mp4rd_moof(a.src, seg, at, size, head, a.x, mo, [&](uint64_t, const Mp4TrunRec& r) {
                if (bad) return;                                     /* (behind a bad sample nothing is looked at: the sums may wrap) */
                if (r.tr & kRdHead) before = 0;
                if (mp4rd_entry_bytes(r.tr) == 0u) {
                    /* entries of no bytes: the count is bounded by nothing in the box, so no loop over it */
                    const uint64_t good = mp4rd_run_good(r.begin, before, r.def_size, a.n, r.tfdt, dur_before, r.def_dur, r.count);
                    if (good < r.count) { bad = k + good + 1; return; }
                    const uint64_t sz = (uint64_t)r.count * r.def_size;
                    before += sz; bytes += sz; dur_before += (uint64_t)r.count * r.def_dur; k += r.count;
                    return;
                }
                for (uint32_t e = 0; e < r.count; ++e, ++k) {            /* (count x 4 bytes or more lie in the box) */
                    const Mp4Sample s = mp4rd_sample(a.src, r, e);
                    uint64_t off, dts, pts;
                    if (!mp4rd_place(r.begin, before, s.size, a.n, r.tfdt, dur_before, s.cts, off, dts, pts)) { bad = k + 1; return; }
                    before += s.size; dur_before += s.dur; bytes += s.size;
                }
            });
        }
        if (MODE == 1) {
            hbs_mp4_frag f;
            f.out_off = at; f.out_bytes = a.moof_span[m]; f.first_au = k0; f.decode_time = mo.tfdt;
            f.samples = (uint32_t)mo.samples; f.sequence = mo.sequence;
            f.flags = (mo.samples && mp4rd_sync(first_flags)) ? (uint32_t)HBS_AU_IRAP : 0u; f.reserved = 0;
            a.frag_tmp[m] = f;
        }
    }
    if (MODE == 2) {
        bad = block_min_nonzero(bad);
        uint64_t bex, btot;
        block_scan<1, kRT>(&bytes, &bex, &btot);
        if (threadIdx.x == 0) { a.part_e[(uint64_t)blockIdx.x * 8] = btot; a.part_e[(uint64_t)blockIdx.x * 8 + 1] = bad; }
    }
}

__global__ __launch_bounds__(kPlanLanes) void k_rd_scan_moof(Mp4RdArgs a, uint64_t moof_blocks)
{
    if (a.ctl[kStop] != 0) return;
    uint64_t carry[2];
    const uint64_t bad = scan_parts<2>(a.part_m, moof_blocks, carry);
    if (threadIdx.x == 0) {
        a.ctl[kTruns] = carry[0]; a.ctl[kSamples] = carry[1]; a.ctl[kBadMoof] = bad;
        if (bad || (a.out && carry[1] > a.sample_cap)) a.ctl[kStop] = 2;
        else if (a.out) a.trun_first[carry[0]] = (uint32_t)carry[1];
    }
}

/* ---- samples ----------------------------------------------------------------------------------------------------------- */

/* MODE 0 count, 1 check, 2 place */
template <int MODE>
__global__ __launch_bounds__(kRT) void k_rd_samp(Mp4RdArgs a)
{
    if (a.ctl[MODE == 2 ? kErr : kStop] != 0) return;
    const uint64_t N = a.ctl[kSamples], T = a.ctl[kTruns];
    const uint64_t k = (uint64_t)blockIdx.x * kRT + threadIdx.x;
    const bool in = k < N;
    uint64_t v[2] = {0, 0};
    bool head[2] = {false, false};
    Mp4Sample s;
    s.dur = 0; s.size = 0; s.flags = 0; s.cts = 0;
    int64_t begin = 0;
    uint64_t tfdt = 0;
    if (in) {
        /* the last trun whose first sample is k or in front of it */
        uint64_t lo = 0, hi = T - 1;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo + 1) / 2;
            if (a.trun_first[mid] <= k) lo = mid; else hi = mid - 1;
        }
        const Mp4TrunRec t = a.trun[lo];
        const uint32_t e = (uint32_t)k - t.first;
        s = mp4rd_sample(a.src, t, e);
        v[0] = s.size; v[1] = s.dur;
        head[0] = e == 0u && (t.tr & kRdHead) != 0u; head[1] = e == 0u && (t.tr & kRdMoofFirst) != 0u;
        begin = t.begin; tfdt = t.tfdt;
    }
    uint64_t ex[2], tot[2];
    bool exf[2], totf[2];
    block_seg_excl<2, kRT>(v, head, ex, exf, tot, totf);
    unsigned long long* part = a.part_k + (uint64_t)blockIdx.x * 8;
    if (MODE == 0) {
        if (threadIdx.x == 0) { part[0] = tot[0]; part[1] = tot[1]; part[2] = totf[0] ? 1 : 0; part[3] = totf[1] ? 1 : 0; }
        return;
    }
    uint64_t before[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) before[q] = head[q] ? 0 : exf[q] ? ex[q] : ex[q] + part[q];
    uint64_t off = 0, dts = 0, pts = 0;
    const bool ok = !in || mp4rd_place(begin, before[0], s.size, a.n, tfdt, before[1], s.cts, off, dts, pts);
    if (MODE == 1) {
        const uint64_t bad = block_min_nonzero(ok ? 0 : k + 1);
        uint64_t bex, btot;
        block_scan<1, kRT>(&v[0], &bex, &btot);
        if (threadIdx.x == 0) { a.part_c[(uint64_t)blockIdx.x * 8] = btot; a.part_c[(uint64_t)blockIdx.x * 8 + 1] = bad; }
        return;
    }
    if (!in) return;
    a.sample_off[k] = off; a.sample_size[k] = s.size;
    if (a.dts) a.dts[k] = dts;
    if (a.pts) a.pts[k] = pts;
    if (a.sample_flags) a.sample_flags[k] = s.flags;
}

__global__ __launch_bounds__(kPlanLanes) void k_rd_scan_samp(Mp4RdArgs a, uint64_t samp_blocks)
{
    if (a.ctl[kStop] != 0) return;
    seg_scan_parts<2>(a.part_k, samp_blocks);
}

__global__ __launch_bounds__(kPlanLanes) void k_rd_finish(Mp4RdArgs a, uint64_t blocks)
{
    const uint64_t stop = a.ctl[kStop];
    uint64_t carry[1] = {0}, bad_sample = 0;
    if (!stop) bad_sample = scan_parts<1>(a.out ? a.part_c : a.part_e, blocks, carry);
    if (threadIdx.x == 0) {
        const uint64_t M = a.ctl[kMoofs], N = a.ctl[kSamples], bad_seg = a.ctl[kBadSeg], bad_moof = a.ctl[kBadMoof];
        hbs_summary s;
        s.nal_count = 0; s.nal_found = 0; s.rbsp_bytes = 0; s.stream_bytes = a.n; s.stop_reason = 0;
        s.reserved[0] = bad_seg; s.reserved[1] = 0; s.reserved[2] = 0;
        int32_t err = 0;
        if (bad_seg) err = HBS_E_ARG;
        else {
            s.nal_found = M;
            if (M > a.moof_cap) err = HBS_E_CAPACITY;
            else if (bad_moof) { err = HBS_E_ARG; s.reserved[1] = bad_moof; }
            else {
                s.nal_count = N;
                if (stop) err = HBS_E_CAPACITY;                        /* (N > sample_cap: the samples were not looked at) */
                else if (bad_sample) { err = HBS_E_ARG; s.reserved[2] = bad_sample; }
                else s.rbsp_bytes = carry[0];
            }
        }
        s.error = err;
        a.ctl[kErr] = err ? 1 : 0;
        *a.summary = s;
    }
}

__global__ __launch_bounds__(kRT) void k_rd_frags(Mp4RdArgs a)
{
    if (a.ctl[kErr] != 0) return;
    const uint64_t m = (uint64_t)blockIdx.x * kRT + threadIdx.x;
    if (m < a.ctl[kMoofs]) a.frag[m] = a.frag_tmp[m];
}

} // namespace

hipError_t launch_mp4_samples(const Mp4RdArgs& a, hipStream_t st)
{
    const uint64_t sb = (a.n_segs + kRT - 1) / kRT, mb = (a.moof_cap + kRT - 1) / kRT, kb = a.out ? (a.sample_cap + kRT - 1) / kRT : 0;
    const hipError_t e = begin_launches(a.ev_begin, st);
    if (e != hipSuccess) return e;
    if (sb) hipLaunchKernelGGL(k_rd_seg<0>, dim3((unsigned)sb), dim3(kRT), 0, st, a);
    hipLaunchKernelGGL(k_rd_scan_seg, dim3(1), dim3(kPlanLanes), 0, st, a, sb);
    if (sb && mb) {
        hipLaunchKernelGGL(k_rd_seg<1>, dim3((unsigned)sb), dim3(kRT), 0, st, a);
        hipLaunchKernelGGL(k_rd_moof<0>, dim3((unsigned)mb), dim3(kRT), 0, st, a);
    }
    hipLaunchKernelGGL(k_rd_scan_moof, dim3(1), dim3(kPlanLanes), 0, st, a, sb ? mb : 0);
    if (sb && mb) {
        if (a.out) hipLaunchKernelGGL(k_rd_moof<1>, dim3((unsigned)mb), dim3(kRT), 0, st, a);
        else hipLaunchKernelGGL(k_rd_moof<2>, dim3((unsigned)mb), dim3(kRT), 0, st, a);
    }
    if (a.out && sb && mb && kb) {
        hipLaunchKernelGGL(k_rd_samp<0>, dim3((unsigned)kb), dim3(kRT), 0, st, a);
        hipLaunchKernelGGL(k_rd_scan_samp, dim3(1), dim3(kPlanLanes), 0, st, a, kb);
        hipLaunchKernelGGL(k_rd_samp<1>, dim3((unsigned)kb), dim3(kRT), 0, st, a);
    }
    const bool ran = sb && mb;
    hipLaunchKernelGGL(k_rd_finish, dim3(1), dim3(kPlanLanes), 0, st, a, !ran ? 0 : a.out ? kb : mb);
    if (a.out && ran) {
        if (kb) hipLaunchKernelGGL(k_rd_samp<2>, dim3((unsigned)kb), dim3(kRT), 0, st, a);
        if (a.frag) hipLaunchKernelGGL(k_rd_frags, dim3((unsigned)mb), dim3(kRT), 0, st, a);
    }
    return end_launches(a.ev_end, st);
}

} // namespace hbs

extern "C" {

int64_t hbs_mp4_init_read_host(const uint8_t* seg, uint64_t n, uint32_t track_id, hbs_mp4_track* out, uint64_t* nal_off, uint64_t* nal_bytes,
                               uint64_t cap)
{
    return hbs::mp4_init_read_host(seg, n, track_id, out, nal_off, nal_bytes, cap);
}

}
