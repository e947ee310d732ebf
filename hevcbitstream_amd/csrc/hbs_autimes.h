/*
 * hbs_autimes.h -- hbs_au_times (include/hevcbitstream_amd.h): the rules as host/device inline functions -- aut_params_ok
 * refuses what the call refuses at once, aut_ukey biases a picture order count to an unsigned key, aut_seg_combine is the
 * operator of every scan of the call (a maximum that restarts at marked elements), aut_back_step / aut_fwd_step are one step
 * of the walk and aut_rank the whole walk of one AU, aut_dts / aut_pts / aut_late the times -- the segmented maximum over the
 * lanes of a workgroup, and the host-visible launcher.  Everything above the device part compiles with plain g++
 * (tests/test_au_times_host_asan.py single-steps the plan with it).
 *
 * One operator serves three scans.  With (f1, x1) o (f2, x2) = (f1 | f2, f2 ? x2 : max(x1, x2)), x = 0 the identity:
 *   the key of the last picture   f = the AU has a picture,           x = its biased key     (a maximum of one element)
 *   pmax, forwards                f = the AU begins a segment,        x = key(a) biased
 *   smin, backwards               f = the AU ends a segment,          x = ~(key(a) biased)   (a minimum is a maximum of complements)
 */
#ifndef HBS_AUTIMES_H
#define HBS_AUTIMES_H

#include "hbs_common.h"

namespace hbs {

constexpr int kAutLanes = 256;                       /* an AU a lane: B = 256 AUs a workgroup                            */
constexpr int kAutHalo = 64;                         /* H: AUs on either side of them the rank kernel stages in LDS      */
constexpr uint32_t kAutFlags = HBS_AUT_DELAY_GIVEN | HBS_AUT_WRAP33;
constexpr uint64_t kAutMaxAus = 0xFFFFFFFFull;
constexpr uint64_t kAutTimeLimit = 1ull << 62;

/* the byte a workgroup keeps per AU */
enum : uint32_t { kAutHead = 1u, kAutPic = 2u, kAutKnown = 4u };     /* begins a segment; has a picture; one lies at or in front of it
                                                                        in its workgroup (its key does not need the carry) */
/* the 8 words a workgroup leaves (k_aut_digest), and what becomes of them */
enum : int {
    kAutPKey = 0,                                    /* the key of its last picture -> of the last picture in front of it     */
    kAutPMax = 1,                                    /* the maximum behind its last head -> pmax of the AU in front of it     */
    kAutPMin = 2,                                    /* ~ the minimum up to its first segment end -> ~ smin of the AU behind it */
    kAutPBits = 3,                                   /* kAutB*                                                                */
    kAutPHeads = 4,                                  /* heads in it -> (k_aut_rank) AUs with pts < dts                        */
    kAutPLast = 5,                                   /* 1 + its last head (0: none)                                           */
    kAutPLag = 6,                                    /* (k_aut_rank) max(a - o(a)), at least 0                                */
    kAutPBad = 7                                     /* (k_aut_rank) 1 + the lowest AU that offends the span limit (0: none)  */
};
enum : uint32_t { kAutBPic = 1u, kAutBHead = 2u, kAutBEnd = 4u, kAutBLead = 8u };   /* a picture, a head, a segment end lies in the workgroup;
                                                                                      its last head has no kAutKnown                */
/* ctl words */
enum : int { kAutCSegs = 0, kAutCLast = 1, kAutCBad = 2, kAutCDelay = 3 };

/* what the call refuses at once.  Every time of the call is below 2^62: base_time + (n_aus + D) * tick, with D the given
 * delay or the largest one the span limit admits */
HBS_HD bool aut_params_ok(const hbs_au_times_params* p, uint64_t n_aus)
{
    if (!p || (p->flags & ~kAutFlags) != 0u || p->reserved[0] != 0u || p->reserved[1] != 0u || p->reserved[2] != 0u) return false;
    if (p->tick == 0u || p->base_time >= kAutTimeLimit || n_aus > kAutMaxAus) return false;
    const uint64_t d = (p->flags & HBS_AUT_DELAY_GIVEN) ? p->delay : HBS_AUT_MAX_SPAN;
    return n_aus + d <= (kAutTimeLimit - 1u - p->base_time) / p->tick;
}

HBS_HD uint32_t aut_ukey(int32_t pic_order_cnt) { return (uint32_t)pic_order_cnt ^ 0x80000000u; }
HBS_HD bool aut_is_head(uint64_t a, uint32_t au_flags) { return a == 0 || (au_flags & HBS_AU_CVS_START) != 0u; }
HBS_HD bool aut_has_picture(uint32_t au_flags) { return (au_flags & HBS_AU_NO_PICTURE) == 0u; }

struct AutSeg { uint32_t f, x; };
HBS_HD AutSeg aut_seg(uint32_t f, uint32_t x) { AutSeg r; r.f = f; r.x = x; return r; }
/* a in front of b */
HBS_HD AutSeg aut_seg_combine(AutSeg a, AutSeg b)
{
    AutSeg r;
    r.f = a.f | b.f;
    r.x = b.f ? b.x : (a.x > b.x ? a.x : b.x);
    return r;
}
/* what an AU gets from the scan: `inc` is the scan over its workgroup up to and including it, `carry` what lies beyond */
HBS_HD uint32_t aut_seg_value(uint32_t carry, AutSeg inc) { return inc.f ? inc.x : (carry > inc.x ? carry : inc.x); }

/* what the walk reads of an AU: biased key, pmax and smin (biased as the key is), whether it begins a segment */
struct AutRec { uint32_t key, pmax, smin, head; };

/* one step of the walk of the AU with key `ka`, backwards at AU b of its segment: false = neither b nor an AU of the segment in
 * front of b has a higher key (pmax is monotone inside a segment) */
HBS_HD bool aut_back_step(uint32_t ka, const AutRec& b, uint32_t& inversions)
{
    if (b.pmax <= ka) return false;
    inversions += b.key > ka ? 1u : 0u;
    return true;
}
/* ... forwards at AU b of its segment: false = neither b nor an AU of the segment behind b has a lower key */
HBS_HD bool aut_fwd_step(uint32_t ka, const AutRec& b, uint32_t& inversions)
{
    if (b.smin >= ka) return false;
    inversions += b.key < ka ? 1u : 0u;
    return true;
}

struct AutRank { uint32_t order, bad; };
/* o(a) by the second form of the specification: rec(b) is AutRec of AU b < n.  The backward walk visits a - 1 ... a - back(a), the
 * forward one a + 1 ... a + fwd(a), and no AU more; one that would take step HBS_AUT_MAX_SPAN + 1 offends */
template <class F> HBS_HD AutRank aut_rank(uint64_t a, uint64_t n, F rec)
{
    const AutRec me = rec(a);
    AutRank r;
    r.bad = 0;
    uint32_t before = 0, behind = 0;
    if (!me.head) {
        for (uint64_t s = 1; s <= a; ++s) {
            const AutRec b = rec(a - s);
            if (!aut_back_step(me.key, b, before)) break;
            if (s > HBS_AUT_MAX_SPAN) { r.bad = 1; break; }      /* (the order of an offending AU is never read) */
            if (b.head) break;
        }
    }
    for (uint64_t s = 1; a + s < n; ++s) {
        const AutRec b = rec(a + s);
        if (b.head || !aut_fwd_step(me.key, b, behind)) break;
        if (s > HBS_AUT_MAX_SPAN) { r.bad = 1; break; }
    }
    r.order = (uint32_t)a + behind - before;
    return r;
}

/* the times: exact below 2^62 (aut_params_ok), then modulo 2^33 when asked */
HBS_HD uint64_t aut_wrap(uint64_t t, uint32_t flags) { return (flags & HBS_AUT_WRAP33) ? (t & ((1ull << 33) - 1u)) : t; }
HBS_HD uint64_t aut_dts(uint64_t base_time, uint32_t tick, uint64_t a, uint32_t flags) { return aut_wrap(base_time + a * tick, flags); }
HBS_HD uint64_t aut_pts(uint64_t base_time, uint32_t tick, uint64_t order, uint64_t delay, uint32_t flags)
{
    return aut_wrap(base_time + (order + delay) * tick, flags);
}
/* exact pts < dts */
HBS_HD bool aut_late(uint64_t a, uint64_t order, uint64_t delay) { return order + delay < a; }
/* a - o(a), 0 where it is negative: R is the maximum of these */
HBS_HD uint32_t aut_lag(uint64_t a, uint64_t order) { return a > order ? (uint32_t)(a - order) : 0u; }

HBS_HD uint64_t aut_blocks(uint64_t n_aus) { return (n_aus + kAutLanes - 1) / kAutLanes; }

#ifdef __HIPCC__
} // namespace hbs
#include <hip/hip_runtime.h>
namespace hbs {

/* the scan of aut_seg_combine over the NT lanes of a workgroup: ex = the lanes in front of this one (f = 0, x = 0 for lane 0),
 * tot = all of them */
template <int NT>
__device__ __forceinline__ void block_segmax_excl(AutSeg v, AutSeg& ex, AutSeg& tot)
{
    __shared__ uint32_t s_x[NT / 64], s_f[NT / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    AutSeg c = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(c.x, (unsigned)d, 64);
        const uint32_t g = __shfl_up(c.f, (unsigned)d, 64);
        if (lane >= d) c = aut_seg_combine(aut_seg(g, y), c);
    }
    if (lane == 63) { s_x[wave] = c.x; s_f[wave] = c.f; }
    const uint32_t y = __shfl_up(c.x, 1u, 64);
    const uint32_t g = __shfl_up(c.f, 1u, 64);
    const AutSeg b = lane ? aut_seg(g, y) : aut_seg(0u, 0u);
    __syncthreads();
    AutSeg p = aut_seg(0u, 0u), all = aut_seg(0u, 0u);
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        const AutSeg e = aut_seg(s_f[w], s_x[w]);
        if (w < wave) p = aut_seg_combine(p, e);
        all = aut_seg_combine(all, e);
    }
    ex = aut_seg_combine(p, b);
    tot = all;
    __syncthreads();
}

struct AutArgs {
    const hbs_access_unit* au; uint64_t n;
    uint32_t flags, tick, delay_given; uint64_t base_time;
    unsigned long long* dts; unsigned long long* pts; uint32_t* order; uint32_t* display;     /* each nullable */
    hbs_summary* summary;
    /* scratch (lay_au_times): 17 bytes an AU, 32 a workgroup */
    uint32_t* key;                  /* n: the biased key of the last picture in the workgroup at or in front of the AU, then key(a) */
    uint32_t* pmax;                 /* n */
    uint32_t* smin;                 /* n */
    uint32_t* ord;                  /* n: o(a) */
    uint8_t* bits;                  /* n: kAutHead | kAutPic | kAutKnown */
    uint32_t* part;                 /* 8 per workgroup: kAutP* */
    uint32_t* ctl;                  /* 64: kAutC* */
    hipEvent_t ev_begin, ev_end;
};
/* the scratch the call needs, sized by a.n alone */
inline void lay_au_times(Carver& w, AutArgs& a)
{
    const uint64_t blocks = aut_blocks(a.n);
    a.key = w.take<uint32_t>(a.n * 4);
    a.pmax = w.take<uint32_t>(a.n * 4);
    a.smin = w.take<uint32_t>(a.n * 4);
    a.ord = w.take<uint32_t>(a.n * 4);
    a.bits = w.take<uint8_t>(a.n);
    a.part = w.take<uint32_t>(blocks * 32);
    a.ctl = w.take<uint32_t>(256);
}
hipError_t launch_au_times(const AutArgs& a, hipStream_t st);
#endif

} // namespace hbs
#endif
