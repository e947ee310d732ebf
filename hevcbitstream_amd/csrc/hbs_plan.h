/* hbs_plan.h -- device-only: the scans of a "count, scan, place" plan (hbs_filter.hip, hbs_lenpref.hip, hbs_ts.hip,
 * hbs_tsmux.hip, hbs_rtp.hip, hbs_rtpun.hip, hbs_rtpord.hip, hbs_auins.hip, hbs_mp4.hip): over the lanes of a workgroup the exclusive sums (block_scan) and
 * the exclusive maxima (block_excl_max).  A count kernel leaves 8 words a workgroup -- N sums, then a word that says what was
 * wrong -- and one workgroup of kPlanLanes lanes turns the sums into offsets (scan_parts). */
#ifndef HBS_PLAN_H
#define HBS_PLAN_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hbs {

constexpr int kPlanLanes = 256;                       /* lanes of the workgroup that runs scan_parts            */
constexpr int kPlanPer = 8;                           /* ... consecutive workgroups' words a lane takes per step */

/* exclusive scan of N sums over the NT lanes of a workgroup; tot = the workgroup's totals */
template <int N, int NT>
__device__ __forceinline__ void block_scan(const uint64_t v[N], uint64_t ex[N], uint64_t tot[N])
{
    __shared__ unsigned long long s_w[NT / 64][N];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t inc[N];
#pragma unroll
    for (int q = 0; q < N; ++q) {
        unsigned long long x = v[q];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long y = __shfl_up(x, (unsigned)d, 64);
            if (lane >= d) x += y;
        }
        inc[q] = x;
        if (lane == 63) s_w[wave][q] = x;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < N; ++q) {
        uint64_t pre = 0, all = 0;
        for (int w = 0; w < NT / 64; ++w) {
            const uint64_t x = s_w[w][q];
            if (w < wave) pre += x;
            all += x;
        }
        ex[q] = pre + inc[q] - v[q];
        tot[q] = all;
    }
    __syncthreads();
}

/* exclusive maximum of N fields over the NT lanes of a workgroup (0, the identity, for lane 0); tot = the maximum of all */
template <class T, int N, int NT>
__device__ __forceinline__ void block_excl_max(const T v[N], T ex[N], T tot[N])
{
    __shared__ T s_w[NT / 64][N];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T before[N];
#pragma unroll
    for (int q = 0; q < N; ++q) {
        T x = v[q];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const T y = __shfl_up(x, (unsigned)d, 64);
            if (lane >= d && y > x) x = y;
        }
        const T y = __shfl_up(x, 1u, 64);
        before[q] = lane ? y : 0;
        if (lane == 63) s_w[wave][q] = x;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < N; ++q) {
        T pre = 0, all = 0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) {
            const T x = s_w[w][q];
            if (w < wave && x > pre) pre = x;
            if (x > all) all = x;
        }
        ex[q] = before[q] > pre ? before[q] : pre;
        tot[q] = all;
    }
    __syncthreads();
}

/* the lowest non-zero `x` of the workgroup's lanes (0: all are zero) */
__device__ __forceinline__ uint64_t block_min_nonzero(uint64_t x)
{
    __shared__ unsigned long long s_min;
    if (threadIdx.x == 0) s_min = ~0ull;
    __syncthreads();
    if (x) atomicMin(&s_min, (unsigned long long)x);
    __syncthreads();
    const uint64_t m = s_min;
    __syncthreads();
    return m == ~0ull ? 0 : m;
}

/* one workgroup of kPlanLanes: the per-workgroup sums part[8 i + 0..N-1] become their exclusive prefix sums, carry their
 * totals; returns the lowest non-zero part[8 i + N] (0: none) */
template <int N>
__device__ __forceinline__ uint64_t scan_parts(unsigned long long* part, uint64_t blocks, uint64_t carry[N])
{
    uint64_t flag = 0;
#pragma unroll
    for (int q = 0; q < N; ++q) carry[q] = 0;
    for (uint64_t seg = 0; seg < blocks; seg += (uint64_t)kPlanLanes * kPlanPer) {
        const uint64_t i0 = seg + (uint64_t)threadIdx.x * kPlanPer;
        uint64_t v[N] = {};
        for (int i = 0; i < kPlanPer && i0 + i < blocks; ++i) {
            const unsigned long long* p = part + (i0 + i) * 8;
#pragma unroll
            for (int q = 0; q < N; ++q) v[q] += p[q];
            if (p[N] && (!flag || p[N] < flag)) flag = p[N];
        }
        uint64_t ex[N], tot[N];
        block_scan<N, kPlanLanes>(v, ex, tot);
#pragma unroll
        for (int q = 0; q < N; ++q) ex[q] += carry[q];
        for (int i = 0; i < kPlanPer && i0 + i < blocks; ++i) {
            unsigned long long* p = part + (i0 + i) * 8;
#pragma unroll
            for (int q = 0; q < N; ++q) { const uint64_t x = p[q]; p[q] = ex[q]; ex[q] += x; }
        }
#pragma unroll
        for (int q = 0; q < N; ++q) carry[q] += tot[q];
    }
    return block_min_nonzero(flag);
}

/* one workgroup of kPlanLanes: the per-workgroup maxima last[i] become the maxima of the workgroups in front, last[i] =
 * max(last[0 .. i)) (0, the identity, for i == 0); returns the maximum of all */
__device__ __forceinline__ uint64_t max_scan_parts(unsigned long long* last, uint64_t blocks)
{
    uint64_t run = 0;
    for (uint64_t seg = 0; seg < blocks; seg += (uint64_t)kPlanLanes * kPlanPer) {
        const uint64_t i0 = seg + (uint64_t)threadIdx.x * kPlanPer;
        uint64_t acc = 0;
        for (int i = 0; i < kPlanPer && i0 + i < blocks; ++i) { const uint64_t x = last[i0 + i]; if (x > acc) acc = x; }
        uint64_t cur, tot;
        block_excl_max<uint64_t, 1, kPlanLanes>(&acc, &cur, &tot);
        if (run > cur) cur = run;
        for (int i = 0; i < kPlanPer && i0 + i < blocks; ++i) {
            const uint64_t x = last[i0 + i];
            last[i0 + i] = cur;
            if (x > cur) cur = x;
        }
        if (tot > run) run = tot;
    }
    return run;
}

} // namespace hbs
#endif
