/*
 * hbs_autimes.hip -- hbs_au_times: decode and presentation times of access units from their picture order counts
 * (include/hevcbitstream_amd.h is the specification, hbs_autimes.h the rules).  Six launches, none of which waits for another
 * workgroup; a workgroup takes kAutLanes = 256 consecutive AUs, one a lane:
 *
 *   k_aut_digest  reads flags and pic_order_cnt of each AU (two words of the 64-byte record), leaves a byte (head, picture,
 *                 "a picture lies at or in front of it in this workgroup") and the key of that picture, and per workgroup the
 *                 aggregates of three scans of aut_seg_combine -- the last picture's key, the maximum behind its last head,
 *                 the minimum up to its first segment end -- with its heads and the last of them
 *   k_aut_parts   one workgroup of kPlanLanes: the aggregates become carries (the third scan runs over the workgroups from the
 *                 back); the segments and the last head go to the control words
 *   k_aut_apply   key(a), pmax(a) and, with the lanes taken in reverse, smin(a)
 *   k_aut_rank    a lane per AU walks backwards while pmax says a higher key lies there and forwards while smin says a lower one
 *                 does (aut_rank): o(a); per workgroup max(a - o(a)), the lowest offending AU, the AUs with pts < dts
 *   k_aut_reduce  one workgroup: R, the error, the delay, the summary
 *   k_aut_write   d_dts, d_pts, d_order, d_display (not launched for a plan; returns at once on the error)
 *
 * An AU in front of its workgroup's first picture does not know its key before k_aut_parts has run (it is the key of the last
 * picture of an earlier workgroup, K).  k_aut_digest leaves such keys out of its aggregates, which is exact but for one case:
 *   backwards  the aggregate only matters to the workgroup in front when this one's first AU is no head; then that workgroup's
 *              last AU lies in the same segment and has key K itself, so K is in its minimum already;
 *   forwards   the same holds when no head lies among those AUs: the carry that comes in is pmax of an AU with key K.  When the
 *              workgroup's LAST head is one of them (a head without a picture: out of spec, but the formulas are the definition)
 *              the segment it begins holds K, and k_aut_parts, which knows K by then, adds it (kAutBLead).
 *
 * Traffic: 64 B an AU read once (the two words share no 32-byte sector with each other, the record is read as one line); 17 B an
 * AU of scratch written, 13 + 16 read (k_aut_apply, k_aut_rank; the walks read LDS, or L2 beyond the halo), 4 rewritten; the
 * outputs asked for.
 */
#include <hip/hip_runtime.h>
#include "hbs_autimes.h"
#include "hbs_plan.h"

namespace hbs {
namespace {

constexpr int kT = kAutLanes;
constexpr int kStage = kT + 2 * kAutHalo;            /* AUs the rank kernel stages */

__global__ __launch_bounds__(kT) void k_aut_digest(AutArgs a)
{
    __shared__ uint32_t s_key[kT];
    __shared__ uint8_t s_bits[kT];
    const int t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kT, k = base + t;
    const bool valid = k < a.n;
    uint32_t flags = HBS_AU_NO_PICTURE, poc = 0;
    if (valid) { flags = a.au[k].flags; poc = (uint32_t)a.au[k].pic_order_cnt; }
    const bool head = valid && aut_is_head(k, flags), pic = valid && aut_has_picture(flags);
    /* 1. the last picture at or in front of the AU */
    AutSeg ex, tot_key, tot_max, tot_min;
    const AutSeg own = aut_seg(pic ? 1u : 0u, pic ? aut_ukey((int32_t)poc) : 0u);
    block_segmax_excl<kT>(own, ex, tot_key);
    const AutSeg last = aut_seg_combine(ex, own);
    const uint32_t key = last.f ? last.x : 0u;       /* 0 is the identity: an AU without a known key takes no part below */
    const uint32_t bits = (head ? kAutHead : 0u) | (pic ? kAutPic : 0u) | (last.f ? kAutKnown : 0u);
    if (valid) { a.key[k] = key; a.bits[k] = (uint8_t)bits; }
    s_key[t] = key; s_bits[t] = (uint8_t)(valid ? bits : 0u);
    /* 2. the maximum behind the last head */
    block_segmax_excl<kT>(aut_seg(head ? 1u : 0u, key), ex, tot_max);
    const int known_head = __syncthreads_or(head && last.f), blind_head = __syncthreads_or(head && !last.f);
    /* 3. from the back: lane t takes AU e = kT - 1 - t; the AU ends a segment when the next one is a head or there is none */
    const int e = kT - 1 - t;
    const uint64_t ke = base + e;
    bool end = false;
    if (ke < a.n) end = ke + 1 == a.n || (e + 1 < kT ? (s_bits[e + 1] & kAutHead) != 0u : aut_is_head(ke + 1, a.au[ke + 1].flags));
    const bool known = (s_bits[e] & kAutKnown) != 0u;
    block_segmax_excl<kT>(aut_seg(end ? 1u : 0u, known ? ~s_key[e] : 0u), ex, tot_min);
    /* 4. heads, and the last of them */
    const uint64_t one = head ? 1u : 0u, mine = head ? k + 1 : 0u;
    uint64_t exs, heads, exm, last_head;
    block_scan<1, kT>(&one, &exs, &heads);
    block_excl_max<uint64_t, 1, kT>(&mine, &exm, &last_head);
    if (t == 0) {
        uint32_t* p = a.part + (uint64_t)blockIdx.x * 8;
        p[kAutPKey] = tot_key.x; p[kAutPMax] = tot_max.x; p[kAutPMin] = tot_min.x;
        p[kAutPBits] = (tot_key.f ? kAutBPic : 0u) | (tot_max.f ? kAutBHead : 0u) | (tot_min.f ? kAutBEnd : 0u) |
                       ((blind_head && !known_head) ? kAutBLead : 0u);
        p[kAutPHeads] = (uint32_t)heads; p[kAutPLast] = (uint32_t)last_head; p[kAutPLag] = 0; p[kAutPBad] = 0;
    }
}

/* one workgroup of kPlanLanes: word `word` of every workgroup's 8 (f: `bit` of its kAutPBits) becomes the scan of the workgroups
 * in front of it -- behind it with `reversed` */
__device__ __forceinline__ void segmax_scan_parts(uint32_t* part, uint64_t blocks, int word, uint32_t bit, bool reversed)
{
    AutSeg run = aut_seg(0u, 0u);
    for (uint64_t seg = 0; seg < blocks; seg += (uint64_t)kPlanLanes * kPlanPer) {
        const uint64_t i0 = seg + (uint64_t)threadIdx.x * kPlanPer;
        AutSeg acc = aut_seg(0u, 0u);
        for (int i = 0; i < kPlanPer && i0 + i < blocks; ++i) {
            const uint32_t* p = part + (reversed ? blocks - 1 - (i0 + i) : i0 + i) * 8;
            acc = aut_seg_combine(acc, aut_seg((p[kAutPBits] & bit) ? 1u : 0u, p[word]));
        }
        AutSeg ex, tot;
        block_segmax_excl<kPlanLanes>(acc, ex, tot);
        AutSeg cur = aut_seg_combine(run, ex);
        for (int i = 0; i < kPlanPer && i0 + i < blocks; ++i) {
            uint32_t* p = part + (reversed ? blocks - 1 - (i0 + i) : i0 + i) * 8;
            const AutSeg el = aut_seg((p[kAutPBits] & bit) ? 1u : 0u, p[word]);
            p[word] = cur.x;
            cur = aut_seg_combine(cur, el);
        }
        run = aut_seg_combine(run, tot);
    }
}

__global__ __launch_bounds__(kPlanLanes) void k_aut_parts(AutArgs a, uint64_t blocks)
{
    segmax_scan_parts(a.part, blocks, kAutPKey, kAutBPic, false);
    __syncthreads();
    /* the segment that a head without a known key began holds the key the workgroup has just been given */
    uint64_t heads = 0, last = 0;
    for (uint64_t i = threadIdx.x; i < blocks; i += kPlanLanes) {
        uint32_t* p = a.part + i * 8;
        if ((p[kAutPBits] & kAutBLead) && p[kAutPKey] > p[kAutPMax]) p[kAutPMax] = p[kAutPKey];
        heads += p[kAutPHeads];
        if (p[kAutPLast] > last) last = p[kAutPLast];
    }
    __syncthreads();
    segmax_scan_parts(a.part, blocks, kAutPMax, kAutBHead, false);
    segmax_scan_parts(a.part, blocks, kAutPMin, kAutBEnd, true);
    uint64_t ex, segs, exm, last_head;
    block_scan<1, kPlanLanes>(&heads, &ex, &segs);
    block_excl_max<uint64_t, 1, kPlanLanes>(&last, &exm, &last_head);
    if (threadIdx.x == 0) { a.ctl[kAutCSegs] = (uint32_t)segs; a.ctl[kAutCLast] = (uint32_t)last_head; }
}

__global__ __launch_bounds__(kT) void k_aut_apply(AutArgs a)
{
    __shared__ uint32_t s_key[kT];
    __shared__ uint8_t s_head[kT];
    const int t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kT, k = base + t;
    const uint32_t* p = a.part + (uint64_t)blockIdx.x * 8;
    const uint32_t carry_key = p[kAutPKey], carry_max = p[kAutPMax], carry_min = p[kAutPMin];
    const bool valid = k < a.n;
    uint32_t key = 0, bits = 0;
    if (valid) {
        bits = a.bits[k];
        key = (bits & kAutKnown) ? a.key[k] : carry_key;
        if (!(bits & kAutKnown)) a.key[k] = key;
    }
    s_key[t] = key; s_head[t] = (uint8_t)(bits & kAutHead);
    AutSeg ex, tot;
    const AutSeg own = aut_seg(bits & kAutHead, key);
    block_segmax_excl<kT>(own, ex, tot);             /* (its first barrier publishes s_key and s_head) */
    if (valid) a.pmax[k] = aut_seg_value(carry_max, aut_seg_combine(ex, own));
    const int e = kT - 1 - t;
    const uint64_t ke = base + e;
    const bool there = ke < a.n;
    bool end = false;
    if (there) end = ke + 1 == a.n || (e + 1 < kT ? s_head[e + 1] != 0 : (a.bits[ke + 1] & kAutHead) != 0u);
    const AutSeg back = aut_seg(end ? 1u : 0u, there ? ~s_key[e] : 0u);
    block_segmax_excl<kT>(back, ex, tot);
    if (there) a.smin[ke] = ~aut_seg_value(carry_min, aut_seg_combine(ex, back));
}

__global__ __launch_bounds__(kT) void k_aut_rank(AutArgs a)
{
    __shared__ uint32_t s_key[kStage], s_pmax[kStage], s_smin[kStage];
    __shared__ uint8_t s_head[kStage];
    const int t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kT, k = base + t;
    /* slot j holds AU base - kAutHalo + j; AUs outside [0, n) are never asked for */
    for (int j = t; j < kStage; j += kT) {
        const uint64_t g = base + (uint64_t)j;
        if (g >= (uint64_t)kAutHalo && g - kAutHalo < a.n) {
            const uint64_t b = g - kAutHalo;
            s_key[j] = a.key[b]; s_pmax[j] = a.pmax[b]; s_smin[j] = a.smin[b]; s_head[j] = (uint8_t)(a.bits[b] & kAutHead);
        }
    }
    __syncthreads();
    uint64_t lag = 0, bad = 0, late = 0;
    if (k < a.n) {
        const AutRank r = aut_rank(k, a.n, [&](uint64_t b) {
            AutRec x;
            const uint64_t j = b + kAutHalo - base;          /* wraps to a large number in front of the staged AUs */
            if (j < (uint64_t)kStage) { x.key = s_key[j]; x.pmax = s_pmax[j]; x.smin = s_smin[j]; x.head = s_head[j]; }
            else { x.key = a.key[b]; x.pmax = a.pmax[b]; x.smin = a.smin[b]; x.head = a.bits[b] & kAutHead; }
            return x;
        });
        a.ord[k] = r.order;
        lag = aut_lag(k, r.order);
        bad = r.bad ? k + 1 : 0;
        late = ((a.flags & HBS_AUT_DELAY_GIVEN) && !r.bad && aut_late(k, r.order, a.delay_given)) ? 1u : 0u;
    }
    uint64_t ex, lag_max, exs, late_sum;
    block_excl_max<uint64_t, 1, kT>(&lag, &ex, &lag_max);
    block_scan<1, kT>(&late, &exs, &late_sum);
    const uint64_t lowest = block_min_nonzero(bad);
    if (t == 0) {
        uint32_t* p = a.part + (uint64_t)blockIdx.x * 8;
        p[kAutPLag] = (uint32_t)lag_max; p[kAutPBad] = (uint32_t)lowest; p[kAutPHeads] = (uint32_t)late_sum;
    }
}

__global__ __launch_bounds__(kPlanLanes) void k_aut_reduce(AutArgs a, uint64_t blocks)
{
    uint64_t lag = 0, bad = 0, late = 0;
    for (uint64_t i = threadIdx.x; i < blocks; i += kPlanLanes) {
        const uint32_t* p = a.part + i * 8;
        if (p[kAutPLag] > lag) lag = p[kAutPLag];
        if (p[kAutPBad] && (!bad || p[kAutPBad] < bad)) bad = p[kAutPBad];
        late += p[kAutPHeads];
    }
    uint64_t ex, R, exs, late_sum;
    block_excl_max<uint64_t, 1, kPlanLanes>(&lag, &ex, &R);
    block_scan<1, kPlanLanes>(&late, &exs, &late_sum);
    const uint64_t lowest = block_min_nonzero(bad);
    if (threadIdx.x != 0) return;
    const uint64_t delay = (a.flags & HBS_AUT_DELAY_GIVEN) ? a.delay_given : R;
    a.ctl[kAutCBad] = (uint32_t)lowest; a.ctl[kAutCDelay] = (uint32_t)delay;
    hbs_summary sm;
    sm.nal_count = lowest ? 0 : a.n;
    sm.nal_found = (lowest || !blocks) ? 0 : a.ctl[kAutCSegs];
    sm.rbsp_bytes = (lowest || !blocks) ? 0 : a.ctl[kAutCLast] - 1u;
    sm.stream_bytes = 0; sm.stop_reason = 0;
    sm.error = lowest ? HBS_E_DEPTH : 0;
    sm.reserved[0] = lowest ? lowest : delay;
    sm.reserved[1] = lowest ? 0 : R;
    sm.reserved[2] = lowest ? 0 : late_sum;
    *a.summary = sm;
}

__global__ __launch_bounds__(kT) void k_aut_write(AutArgs a)
{
    if (a.ctl[kAutCBad] != 0) return;
    const uint64_t k = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (k >= a.n) return;
    const uint64_t o = a.ord[k], delay = a.ctl[kAutCDelay];
    if (a.dts) a.dts[k] = aut_dts(a.base_time, a.tick, k, a.flags);
    if (a.pts) a.pts[k] = aut_pts(a.base_time, a.tick, o, delay, a.flags);
    if (a.order) a.order[k] = (uint32_t)o;
    if (a.display && o < a.n) a.display[o] = (uint32_t)k;      /* (o is a permutation of [0, n): the comparison only keeps the store in the table) */
}

} // namespace

hipError_t launch_au_times(const AutArgs& a, hipStream_t st)
{
    const uint64_t blocks = aut_blocks(a.n);
    const hipError_t e = begin_launches(a.ev_begin, st);
    if (e != hipSuccess) return e;
    if (blocks) {
        hipLaunchKernelGGL(k_aut_digest, dim3((unsigned)blocks), dim3(kT), 0, st, a);
        hipLaunchKernelGGL(k_aut_parts, dim3(1), dim3(kPlanLanes), 0, st, a, blocks);
        hipLaunchKernelGGL(k_aut_apply, dim3((unsigned)blocks), dim3(kT), 0, st, a);
        hipLaunchKernelGGL(k_aut_rank, dim3((unsigned)blocks), dim3(kT), 0, st, a);
    }
    hipLaunchKernelGGL(k_aut_reduce, dim3(1), dim3(kPlanLanes), 0, st, a, blocks);
    if (blocks && (a.dts || a.pts || a.order || a.display)) hipLaunchKernelGGL(k_aut_write, dim3((unsigned)blocks), dim3(kT), 0, st, a);
    return end_launches(a.ev_end, st);
}

} // namespace hbs
