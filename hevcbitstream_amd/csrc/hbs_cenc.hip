/*
 * hbs_cenc.hip -- hbs_cenc_subsamples and hbs_cenc_crypt: the subsample table of ISO/IEC 23001-7 from the NAL index, and
 * AES-128-CTR in place over the protected ranges (include/hevcbitstream_amd.h is the specification, hbs_cenc.h the rules).
 * No launch waits for another workgroup.
 *
 * hbs_cenc_subsamples, a lane per 8 consecutive NALs, 256 lanes a workgroup:
 *   k_cenc_runs      every check that is about a NAL; the clear count a NAL adds and what it protects.  The running clear count
 *                    is a sum that restarts at an AU's first NAL and behind a NAL that protects something: per workgroup the
 *                    sum of its last run and whether a run begins in it
 *   k_cenc_carry     one workgroup: the sum each workgroup's first lane continues (seg_scan_parts)
 *   k_cenc_count     the same NALs with that sum: the entries each leaves; per workgroup entries, protected bytes, sample bytes, kept
 *   k_cenc_plan      one workgroup: offsets of those, the error, the summary
 *   k_cenc_place     the same NALs once more: d_sub_first at an AU's first NAL, the entries
 *
 * hbs_cenc_crypt.  The entries are as many as d_sub_first[n_samples] says, which the host never learns, so no scratch is sized
 * by them: they are walked in kCencRanges equal ranges, and everything kept is per sample, per range or per workgroup.
 *   k_cenc_samples   a lane a sample: it lies in the buffer and in front of the next, d_sub_first rises from 0
 *   k_cenc_begin     one workgroup: the verdict so far; the entries E (0 after an error: nothing below reads d_sub then)
 *   k_cenc_range_sum a workgroup a range: its bytes and protected bytes, the lowest sample with a clear count above 65535
 *   k_cenc_range_scan one workgroup: the bytes B and protected bytes K in front of every range
 *   k_cenc_at        a workgroup a range, 256 entries a step: B and K at each sample's first entry (at_b, at_k)
 *   k_cenc_sizes     a lane a sample: its entries add up to its size (at_b[s + 1] - at_b[s])
 *   k_cenc_verdict   one workgroup: the error, the summary
 *                    (these seven are enqueue_cenc_checks: hbs_cbcs_crypt, hbs_cbcs.hip, begins with them too)
 *   k_cenc_iv        iv_mode 1 with a d_iv: the counter blocks
 *   k_cenc_crypt     a workgroup per 64 KiB of the protected bytes of all samples, numbered end to end (K).  It finds the range
 *                    its first byte lies in, walks that range's entries 256 a step to where its bytes begin -- their K and their
 *                    place in d_data go to LDS -- and every lane takes the keystream blocks that BEGIN in its 16-byte windows of
 *                    K: one as a rule, two where a sample begins, so no block is computed twice.  A block inside one protected
 *                    range is one 16-byte load, XOR and store at the range's own byte address; one that straddles entries, and
 *                    a sample's last, goes byte by byte along the entries.  Nothing but protected bytes is stored.
 * AES: one table Te0 of 256 words in LDS, filled once a workgroup (cenc_te0); the other three tables are rotations of a looked-up
 * word; the round keys are kernel arguments.
 */
#include <hip/hip_runtime.h>
#include "hbs_cenc.h"
#include "hbs_plan.h"
#include "hbs_copy16.h"

namespace hbs {
namespace {

constexpr int kT = kPlanLanes;
static_assert(kCencNalsPerBlock == kT * kCencNalsPer, "a lane takes kCencNalsPer NALs");

/* ---- hbs_cenc_subsamples ---------------------------------------------------------------------------------------------- */

struct PNal {
    uint64_t clear, protect, rec;      /* 0 for a NAL that is not kept */
    uint32_t raw_au;
    bool bad, kept, first_of_au, last_of_au;
};

/* what a kept NAL with a consistent entry adds and protects */
__device__ __forceinline__ CencNal split_nal(const CencPlanArgs& a, uint64_t k, const hbs_nal_entry& e)
{
    const uint32_t type = e.end > e.start ? ((uint32_t)a.src[e.start] >> 1) & 63u : 63u;
    return cenc_nal_split(a.L, e.start, e.end, type, a.payload_off != nullptr, a.payload_off ? a.payload_off[k] : 0, a.clear_lead, a.flags);
}

__device__ __forceinline__ bool entry_kept(const CencPlanArgs& a, uint64_t k, const hbs_nal_entry& e, uint64_t prev_end)
{
    if (e.start > e.end || e.end > a.n || e.start < prev_end) return false;
    if (a.keep && a.keep[k] == 0) return false;
    return ((e.end - e.start) >> (8u * a.L)) == 0;
}

/* entry k with the end of entry k-1 (0 for k = 0) and the AU word of NAL k-1: every check of the call that is about NAL k */
__device__ __forceinline__ PNal eval_nal(const CencPlanArgs& a, uint64_t k, uint64_t prev_end, uint32_t prev_au)
{
    const hbs_nal_entry e = a.index[k];
    PNal r;
    r.bad = e.start > e.end || e.end > a.n || e.start < prev_end;
    r.kept = entry_kept(a, k, e, prev_end);
    if (!r.bad && !r.kept && (!a.keep || a.keep[k] != 0)) r.bad = true;          /* a kept record too long for L */
    r.raw_au = a.nal_au[k];
    r.first_of_au = k == 0 || r.raw_au != prev_au;
    if (k != 0 && r.raw_au - prev_au > 1u) r.bad = true;
    if (k == a.n_nals - 1 && (uint64_t)(r.raw_au - a.nal_au[0]) + 1 != a.n_aus) r.bad = true;
    r.last_of_au = k == a.n_nals - 1 || a.nal_au[k + 1] != r.raw_au;
    r.clear = r.protect = r.rec = 0;
    if (r.kept) {
        const CencNal c = split_nal(a, k, e);
        if (c.bad) r.bad = true;
        else { r.clear = c.clear; r.protect = c.protect; }
        r.rec = a.L + (e.end - e.start);
    }
    return r;
}

/* the lane's NALs [base, base + kCencNalsPer): x[i], whether a run begins at each, the sum of its last run and whether one
 * begins in it at all; 1 + its lowest bad NAL */
struct LaneNals {
    PNal x[kCencNalsPer];
    bool head[kCencNalsPer];
    uint64_t sum, bad;
    bool any_head;
};

__device__ __forceinline__ void load_lane(const CencPlanArgs& a, uint64_t base, LaneNals& l)
{
    l.sum = 0; l.bad = 0; l.any_head = false;
    const bool in = base < a.n_nals;
    uint64_t prev = 0;
    uint32_t pau = 0;
    bool tprev = false;                       /* the NAL in front protects something: a run ended with it */
    if (in && base) {
        const hbs_nal_entry p = a.index[base - 1];
        prev = p.end; pau = a.nal_au[base - 1];
        const uint64_t pp = base > 1 ? a.index[base - 2].end : 0;
        if (entry_kept(a, base - 1, p, pp)) { const CencNal c = split_nal(a, base - 1, p); tprev = !c.bad && c.protect != 0; }
    }
#pragma unroll
    for (int i = 0; i < kCencNalsPer; ++i) {
        l.x[i].kept = false; l.x[i].first_of_au = false; l.x[i].last_of_au = false; l.x[i].bad = false;
        l.x[i].clear = l.x[i].protect = l.x[i].rec = 0; l.x[i].raw_au = 0;
        l.head[i] = false;
        if (base + i < a.n_nals) {
            l.x[i] = eval_nal(a, base + i, prev, pau);
            prev = a.index[base + i].end; pau = l.x[i].raw_au;
            if (l.x[i].bad && !l.bad) l.bad = base + i + 1;
            l.head[i] = l.x[i].first_of_au || tprev;
            tprev = l.x[i].protect != 0;
            if (l.head[i]) { l.sum = l.x[i].clear; l.any_head = true; }
            else l.sum += l.x[i].clear;
        }
    }
}

/* with `run`, the clear count the lane's first NAL continues: R[i] = the running clear count with NAL i's own bytes in it, and
 * the entries each NAL leaves */
__device__ __forceinline__ void lane_entries(const LaneNals& l, uint64_t run, uint64_t R[kCencNalsPer], uint64_t E[kCencNalsPer])
{
#pragma unroll
    for (int i = 0; i < kCencNalsPer; ++i) {
        run = l.head[i] ? l.x[i].clear : run + l.x[i].clear;
        R[i] = run;
        E[i] = cenc_nal_entries(run, l.x[i].protect, l.x[i].last_of_au);
    }
}

__global__ __launch_bounds__(kT) void k_cenc_runs(CencPlanArgs a)
{
    const uint64_t base = (uint64_t)blockIdx.x * kCencNalsPerBlock + (uint64_t)threadIdx.x * kCencNalsPer;
    LaneNals l;
    load_lane(a, base, l);
    const uint64_t bad = block_min_nonzero(l.bad);
    uint64_t ex, tot;
    bool exf, totf;
    block_seg_excl<1, kT>(&l.sum, &l.any_head, &ex, &exf, &tot, &totf);
    if (threadIdx.x == 0) {
        unsigned long long* p = a.part_a + (uint64_t)blockIdx.x * 8;
        p[0] = tot; p[1] = totf ? 1 : 0; p[2] = bad;
    }
}

__global__ __launch_bounds__(kPlanLanes) void k_cenc_carry(CencPlanArgs a, uint64_t blocks)
{
    seg_scan_parts<1>(a.part_a, blocks);
}

/* the lane's NALs with the running clear count that reaches its first one */
__device__ __forceinline__ void lane_with_run(const CencPlanArgs& a, uint64_t base, LaneNals& l, uint64_t R[kCencNalsPer], uint64_t E[kCencNalsPer])
{
    load_lane(a, base, l);
    uint64_t ex, tot;
    bool exf, totf;
    block_seg_excl<1, kT>(&l.sum, &l.any_head, &ex, &exf, &tot, &totf);
    lane_entries(l, exf ? ex : ex + a.part_a[(uint64_t)blockIdx.x * 8], R, E);
}

__global__ __launch_bounds__(kT) void k_cenc_count(CencPlanArgs a)
{
    const uint64_t base = (uint64_t)blockIdx.x * kCencNalsPerBlock + (uint64_t)threadIdx.x * kCencNalsPer;
    LaneNals l;
    uint64_t R[kCencNalsPer], E[kCencNalsPer];
    lane_with_run(a, base, l, R, E);
    uint64_t v[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < kCencNalsPer; ++i) { v[0] += E[i]; v[1] += l.x[i].protect; v[2] += l.x[i].rec; v[3] += l.x[i].kept ? 1u : 0u; }
    uint64_t ex[4], tot[4];
    block_scan<4, kT>(v, ex, tot);
    if (threadIdx.x == 0) {
        unsigned long long* p = a.part_b + (uint64_t)blockIdx.x * 8;
        p[0] = tot[0]; p[1] = tot[1]; p[2] = tot[2]; p[3] = tot[3];
        p[4] = a.part_a[(uint64_t)blockIdx.x * 8 + 2];
    }
}

__global__ __launch_bounds__(kPlanLanes) void k_cenc_plan(CencPlanArgs a, uint64_t blocks)
{
    uint64_t carry[4];
    const uint64_t bad = scan_parts<4>(a.part_b, blocks, carry);
    if (threadIdx.x == 0) {
        const int32_t err = bad ? HBS_E_ARG : (a.sub && carry[0] > a.sub_cap) ? HBS_E_CAPACITY : 0;
        a.ctl[0] = (unsigned long long)(uint32_t)err;
        if (!err) a.sub_first[a.n_aus] = carry[0];
        hbs_summary s;
        s.nal_count = carry[0]; s.nal_found = a.n_nals; s.rbsp_bytes = carry[1]; s.stream_bytes = carry[2];
        s.stop_reason = 0; s.error = err;
        s.reserved[0] = bad; s.reserved[1] = 0; s.reserved[2] = carry[3];
        *a.summary = s;
    }
}

__global__ __launch_bounds__(kT) void k_cenc_place(CencPlanArgs a)
{
    if (a.ctl[0] != 0) return;
    const uint64_t base = (uint64_t)blockIdx.x * kCencNalsPerBlock + (uint64_t)threadIdx.x * kCencNalsPer;
    LaneNals l;
    uint64_t R[kCencNalsPer], E[kCencNalsPer];
    lane_with_run(a, base, l, R, E);
    uint64_t v = 0, off, tot;
#pragma unroll
    for (int i = 0; i < kCencNalsPer; ++i) v += E[i];
    block_scan<1, kT>(&v, &off, &tot);
    if (base >= a.n_nals) return;
    off += a.part_b[(uint64_t)blockIdx.x * 8];
    const uint32_t au0 = a.nal_au[0];
#pragma unroll
    for (int i = 0; i < kCencNalsPer; ++i) {
        if (base + i >= a.n_nals) break;
        if (l.x[i].first_of_au) a.sub_first[l.x[i].raw_au - au0] = off;            /* (the AU numbers were checked: below n_aus) */
        if (a.sub) for (uint64_t j = 0; j < E[i]; ++j) a.sub[off + j] = cenc_entry(R[i], l.x[i].protect, j, E[i]);
        off += E[i];
    }
}

/* ---- hbs_cenc_crypt ---------------------------------------------------------------------------------------------------- */

__global__ __launch_bounds__(kT) void k_cenc_samples(CencArgs a)
{
    const uint64_t s = (uint64_t)blockIdx.x * kT + threadIdx.x;
    uint64_t bad = 0;
    if (s < a.n_samples) {
        const bool next = s + 1 < a.n_samples;
        if (!cenc_sample_ok(s, a.sample_off[s], a.sample_size[s], next, next ? a.sample_off[s + 1] : 0, a.n, a.sub_first[s], a.sub_first[s + 1]))
            bad = s + 1;
    }
    bad = block_min_nonzero(bad);
    if (threadIdx.x == 0) a.part_s[(uint64_t)blockIdx.x * 8] = bad;
}

/* one workgroup of kPlanLanes: the lowest non-zero part_s word */
__device__ __forceinline__ uint64_t lowest_bad_sample(const CencArgs& a)
{
    return min_nonzero_of<8>(a.part_s, (a.n_samples + kT - 1) / kT);
}

__global__ __launch_bounds__(kPlanLanes) void k_cenc_begin(CencArgs a)
{
    const uint64_t bad = lowest_bad_sample(a);
    if (threadIdx.x == 0) {
        a.ctl[kCencCBad] = bad;
        a.ctl[kCencCEntries] = (bad || !a.n_samples) ? 0 : a.sub_first[a.n_samples];
    }
}

/* the sample entry e belongs to: the last s with d_sub_first[s] <= e */
__device__ __forceinline__ uint64_t sample_of_entry(const CencArgs& a, uint64_t e)
{
    return last_le((uint64_t)0, a.n_samples - 1, e, [&](uint64_t i) { return (uint64_t)a.sub_first[i]; });
}

__global__ __launch_bounds__(kT) void k_cenc_range_sum(CencArgs a)
{
    const uint64_t E = a.ctl[kCencCEntries];
    const uint64_t lo = cenc_range_begin(E, blockIdx.x, kCencRanges), hi = cenc_range_begin(E, blockIdx.x + 1, kCencRanges);
    uint64_t v[2] = {0, 0}, bad = 0;
    for (uint64_t e = lo + threadIdx.x; e < hi; e += kT) {
        const hbs_cenc_subsample x = a.sub[e];
        v[0] += (uint64_t)x.clear + x.protect; v[1] += x.protect;
        if (x.clear > kCencMaxClear && !bad) bad = e + 1;
    }
    bad = block_min_nonzero(bad);
    uint64_t ex[2], tot[2];
    block_scan<2, kT>(v, ex, tot);
    if (threadIdx.x == 0) {
        unsigned long long* p = a.part_r + (uint64_t)blockIdx.x * 8;
        p[0] = tot[0]; p[1] = tot[1]; p[2] = bad ? sample_of_entry(a, bad - 1) + 1 : 0;
    }
}

__global__ __launch_bounds__(kPlanLanes) void k_cenc_range_scan(CencArgs a)
{
    uint64_t carry[2];
    const uint64_t bad = scan_parts<2>(a.part_r, kCencRanges, carry);
    if (threadIdx.x == 0) {
        a.part_r[(uint64_t)kCencRanges * 8] = carry[0]; a.part_r[(uint64_t)kCencRanges * 8 + 1] = carry[1];
        a.ctl[kCencCProt] = carry[1];
        if (!a.ctl[kCencCBad]) a.ctl[kCencCBad] = bad;
    }
}

__global__ __launch_bounds__(kT) void k_cenc_at(CencArgs a)
{
    __shared__ unsigned long long s_b[kT + 1], s_k[kT + 1];
    if (a.ctl[kCencCBad] != 0) return;
    const uint64_t E = a.ctl[kCencCEntries];
    if (E == 0) {                              /* no entry at all: every sample begins at 0 */
        if (blockIdx.x == 0) for (uint64_t s = threadIdx.x; s <= a.n_samples; s += kT) { a.at_b[s] = 0; a.at_k[s] = 0; }
        return;
    }
    const uint64_t lo = cenc_range_begin(E, blockIdx.x, kCencRanges), hi = cenc_range_begin(E, blockIdx.x + 1, kCencRanges);
    uint64_t run[2] = {a.part_r[(uint64_t)blockIdx.x * 8], a.part_r[(uint64_t)blockIdx.x * 8 + 1]};
    for (uint64_t e0 = lo; e0 < hi; e0 += kT) {
        const uint32_t cnt = hi - e0 < (uint64_t)kT ? (uint32_t)(hi - e0) : (uint32_t)kT;
        uint64_t v[2] = {0, 0}, ex[2], tot[2];
        if (threadIdx.x < cnt) { const hbs_cenc_subsample x = a.sub[e0 + threadIdx.x]; v[0] = (uint64_t)x.clear + x.protect; v[1] = x.protect; }
        block_scan<2, kT>(v, ex, tot);
        s_b[threadIdx.x] = run[0] + ex[0]; s_k[threadIdx.x] = run[1] + ex[1];
        if (threadIdx.x == 0) { s_b[cnt] = run[0] + tot[0]; s_k[cnt] = run[1] + tot[1]; }
        __syncthreads();
        /* the samples whose first entry is one of these -- or, behind the last entry of all, the end */
        const uint64_t stop = e0 + cnt + (e0 + cnt == E ? 1u : 0u);
        uint64_t s0 = 0, s1 = a.n_samples + 1;                         /* the first s with d_sub_first[s] >= e0 */
        while (s0 < s1) { const uint64_t m = (s0 + s1) >> 1; if (a.sub_first[m] < e0) s0 = m + 1; else s1 = m; }
        for (uint64_t s = s0 + threadIdx.x; s <= a.n_samples; s += kT) {
            const uint64_t f = a.sub_first[s];
            if (f >= stop) break;
            a.at_b[s] = s_b[f - e0]; a.at_k[s] = s_k[f - e0];
        }
        __syncthreads();
        run[0] += tot[0]; run[1] += tot[1];
    }
}

__global__ __launch_bounds__(kT) void k_cenc_sizes(CencArgs a)
{
    const uint64_t s = (uint64_t)blockIdx.x * kT + threadIdx.x;
    uint64_t bad = 0;
    if (a.ctl[kCencCBad] == 0 && s < a.n_samples && a.at_b[s + 1] - a.at_b[s] != a.sample_size[s]) bad = s + 1;
    bad = block_min_nonzero(bad);
    if (threadIdx.x == 0) a.part_s[(uint64_t)blockIdx.x * 8] = bad;
}

__global__ __launch_bounds__(kPlanLanes) void k_cenc_verdict(CencArgs a)
{
    uint64_t bad = lowest_bad_sample(a);
    if (threadIdx.x == 0) {
        if (a.ctl[kCencCBad]) bad = a.ctl[kCencCBad];
        a.ctl[kCencCErr] = bad ? 1 : 0;
        hbs_summary s;
        s.nal_count = bad ? 0 : a.ctl[kCencCEntries]; s.nal_found = a.n_samples;
        s.rbsp_bytes = bad ? 0 : a.ctl[kCencCProt]; s.stream_bytes = a.n;
        s.stop_reason = 0; s.error = bad ? HBS_E_ARG : 0;
        s.reserved[0] = bad; s.reserved[1] = s.reserved[2] = 0;
        *a.summary = s;
    }
}

__global__ __launch_bounds__(kT) void k_cenc_iv(CencArgs a)
{
    if (a.ctl[kCencCErr] != 0) return;
    const uint64_t s = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (s < a.n_samples) cenc_ctr_store(cenc_ctr_seq(a.iv_base, s), a.iv + 16 * s);
}

/* sample s's counter block */
__device__ __forceinline__ CencCtr sample_ctr(const CencArgs& a, uint64_t s)
{
    if (a.iv_mode) return cenc_ctr_seq(a.iv_base, s);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(a.iv + 16 * s);
    CencCtr c;
    c.hi = ((uint64_t)__builtin_bswap32(w[0]) << 32) | __builtin_bswap32(w[1]);
    c.lo = ((uint64_t)__builtin_bswap32(w[2]) << 32) | __builtin_bswap32(w[3]);
    return c;
}

__global__ __launch_bounds__(kT) void k_cenc_crypt(CencArgs a, CencKey key)
{
    __shared__ uint32_t s_te[256];
    __shared__ unsigned long long s_k[kT + 1], s_p[kT];
    if (a.ctl[kCencCErr] != 0) return;
    const uint64_t all = a.ctl[kCencCProt], E = a.ctl[kCencCEntries];
    const uint64_t t0 = (uint64_t)blockIdx.x * kCencTileBytes;
    if (t0 >= all) return;
    const uint64_t t1 = all - t0 < kCencTileBytes ? all : t0 + kCencTileBytes;
    static_assert(kT == 256, "a lane fills one word of Te0");
    s_te[threadIdx.x] = cenc_te0(threadIdx.x);
    const auto te0 = [&](uint32_t x) { return s_te[x]; };
    /* the last range whose first protected byte is at or in front of the tile's */
    const uint32_t g = last_le(0u, kCencRanges - 1u, t0, [&](uint32_t i) { return (uint64_t)a.part_r[(uint64_t)i * 8 + 1]; });
    uint64_t e = cenc_range_begin(E, g, kCencRanges);
    uint64_t Bc = a.part_r[(uint64_t)g * 8], Kc = a.part_r[(uint64_t)g * 8 + 1];
    const uint64_t last = a.n_samples - 1;
    __syncthreads();
    while (e < E && Kc < t1) {
        const uint32_t cnt = E - e < (uint64_t)kT ? (uint32_t)(E - e) : (uint32_t)kT;
        uint64_t v[2] = {0, 0}, ex[2], tot[2];
        uint32_t clear = 0;
        if (threadIdx.x < cnt) { const hbs_cenc_subsample x = a.sub[e + threadIdx.x]; clear = x.clear; v[0] = (uint64_t)x.clear + x.protect; v[1] = x.protect; }
        block_scan<2, kT>(v, ex, tot);
        const uint64_t Kend = Kc + tot[1];
        if (Kend > t0) {
            s_k[threadIdx.x] = Kc + ex[1]; s_p[threadIdx.x] = Bc + ex[0] + clear;
            if (threadIdx.x == 0) s_k[cnt] = Kend;
            __syncthreads();
            uint64_t s = 0;
#pragma unroll 1
            for (uint64_t w = t0 + 16u * threadIdx.x; w < t1; w += 16u * kT) {
                /* the keystream blocks that begin in [w, w + 16): of the sample w lies in, then of those that begin behind w */
                const uint64_t wend = w + 16u < t1 ? w + 16u : t1;
                s = last_le(s, last, w, [&](uint64_t i) { return (uint64_t)a.at_k[i]; });
                uint64_t b = a.at_k[s] + ((w - a.at_k[s] + 15u) & ~15ull);
#pragma unroll 1
                for (;;) {
                    const uint64_t send = a.at_k[s + 1];
                    if (b < send && b < wend && b >= Kc && b < Kend) {
                        const uint32_t len = send - b < 16u ? (uint32_t)(send - b) : 16u;
                        uint32_t in[4], ks[4];
                        cenc_ctr_block(sample_ctr(a, s), (b - a.at_k[s]) >> 4, in);
                        cenc_aes_block(key, in, ks, te0);
                        const uint32_t i = last_le(0u, cnt - 1u, b, [&](uint32_t q) { return (uint64_t)s_k[q]; });
                        uint64_t pos = a.sample_off[s] - a.at_b[s] + s_p[i] + (b - s_k[i]);
                        uint64_t rem = s_k[i + 1] - b;
                        if (len == 16u && rem >= 16u) {
                            u32x4_u1* p = reinterpret_cast<u32x4_u1*>(a.data + pos);
                            u32x4 d = *p;
                            d.x ^= __builtin_bswap32(ks[0]); d.y ^= __builtin_bswap32(ks[1]);
                            d.z ^= __builtin_bswap32(ks[2]); d.w ^= __builtin_bswap32(ks[3]);
                            *p = d;
                        } else {
                            uint64_t ent = e + i;
                            uint32_t q = 0;
#pragma unroll 1
                            while (q < len) {
                                if (rem == 0) { ent += 1; const hbs_cenc_subsample x = a.sub[ent]; pos += x.clear; rem = x.protect; continue; }
                                a.data[pos] = (uint8_t)(a.data[pos] ^ cenc_block_byte(ks, q));
                                pos += 1; rem -= 1; q += 1;
                            }
                        }
                    }
                    if (send >= wend || s == last) break;
                    s = last_le(s + 1, last, send, [&](uint64_t i) { return (uint64_t)a.at_k[i]; });
                    b = a.at_k[s];
                    if (b >= wend) break;
                }
            }
            __syncthreads();
        }
        e += cnt; Kc = Kend; Bc += tot[0];
    }
}

} // namespace

hipError_t launch_cenc_subsamples(const CencPlanArgs& a, hipStream_t st)
{
    const uint64_t blocks = (a.n_nals + kCencNalsPerBlock - 1) / kCencNalsPerBlock;
    const hipError_t e = begin_launches(a.ev_begin, st);
    if (e != hipSuccess) return e;
    if (blocks) {
        hipLaunchKernelGGL(k_cenc_runs, dim3((unsigned)blocks), dim3(kT), 0, st, a);
        hipLaunchKernelGGL(k_cenc_carry, dim3(1), dim3(kPlanLanes), 0, st, a, blocks);
        hipLaunchKernelGGL(k_cenc_count, dim3((unsigned)blocks), dim3(kT), 0, st, a);
    }
    hipLaunchKernelGGL(k_cenc_plan, dim3(1), dim3(kPlanLanes), 0, st, a, blocks);
    if (blocks) hipLaunchKernelGGL(k_cenc_place, dim3((unsigned)blocks), dim3(kT), 0, st, a);
    return end_launches(a.ev_end, st);
}

void enqueue_cenc_checks(const CencArgs& a, hipStream_t st)
{
    const uint64_t blocks = (a.n_samples + kT - 1) / kT;
    if (blocks) hipLaunchKernelGGL(k_cenc_samples, dim3((unsigned)blocks), dim3(kT), 0, st, a);
    hipLaunchKernelGGL(k_cenc_begin, dim3(1), dim3(kPlanLanes), 0, st, a);
    hipLaunchKernelGGL(k_cenc_range_sum, dim3(kCencRanges), dim3(kT), 0, st, a);
    hipLaunchKernelGGL(k_cenc_range_scan, dim3(1), dim3(kPlanLanes), 0, st, a);
    hipLaunchKernelGGL(k_cenc_at, dim3(kCencRanges), dim3(kT), 0, st, a);
    if (blocks) hipLaunchKernelGGL(k_cenc_sizes, dim3((unsigned)blocks), dim3(kT), 0, st, a);
    hipLaunchKernelGGL(k_cenc_verdict, dim3(1), dim3(kPlanLanes), 0, st, a);
}

hipError_t launch_cenc_crypt(const CencCall& c, hipStream_t st)
{
    const CencArgs& a = c;
    const uint64_t blocks = (a.n_samples + kT - 1) / kT;
    const hipError_t e = begin_launches(a.ev_begin, st);
    if (e != hipSuccess) return e;
    enqueue_cenc_checks(a, st);
    if (blocks && a.iv_mode && a.iv) hipLaunchKernelGGL(k_cenc_iv, dim3((unsigned)blocks), dim3(kT), 0, st, a);
    if (blocks && a.tiles) hipLaunchKernelGGL(k_cenc_crypt, dim3((unsigned)a.tiles), dim3(kT), 0, st, a, c.key);
    return end_launches(a.ev_end, st);
}

} // namespace hbs
