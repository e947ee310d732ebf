/* hbs_plan.h -- device-only: the scans of a "count, scan, place" plan (hbs_filter.hip, hbs_lenpref.hip, hbs_ts.hip,
 * hbs_tsmux.hip, hbs_rtp.hip, hbs_rtpun.hip, hbs_rtpord.hip, hbs_auins.hip, hbs_autimes.hip, hbs_cenc.hip, hbs_cbcs.hip, hbs_mp4.hip, hbs_mp4rd.hip, hbs_mp4stbl.hip, hbs_mp4stblw.hip,
 * hbs_mp4prot.hip, hbs_mp4senc.hip): over the lanes of a workgroup the exclusive sums (block_scan), the exclusive maxima (block_excl_max), the lowest error mark (block_min_nonzero, and min_nonzero_of
 * over the marks that the workgroups left) and the sums that restart at marked lanes (block_seg_excl, seg_scan_parts).  A count kernel leaves 8 words a workgroup -- N sums, then a word that says what
 * was wrong -- and one workgroup of kPlanLanes lanes turns the sums into offsets (scan_parts). */
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

/* one workgroup of kPlanLanes: the lowest non-zero of the words flags[STRIDE i], i < blocks (0: all are zero) */
template <int STRIDE = 1>
__device__ __forceinline__ uint64_t min_nonzero_of(const unsigned long long* flags, uint64_t blocks)
{
    uint64_t m = 0;
    for (uint64_t i = threadIdx.x; i < blocks; i += kPlanLanes) {
        const uint64_t x = flags[i * STRIDE];
        if (x && (!m || x < m)) m = x;
    }
    return block_min_nonzero(m);
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

/* SEGMENTED sums: a lane's value belongs to the run that the nearest lane at or in front of it with `head` set begins (the
 * workgroup's first lanes: to a run that began in a workgroup in front).  ex = the sum of the lanes in front of this one that
 * belong to the run it would continue, exf = whether a head lies among the lanes in front; tot / totf = the same behind the
 * workgroup's last lane: the sum of its last run, and whether any lane began one.  (f, x) pairs under
 * (f1, x1) o (f2, x2) = (f1 | f2, f2 ? x2 : x1 + x2), which is associative. */
template <int N, int NT>
__device__ __forceinline__ void block_seg_excl(const uint64_t v[N], const bool head[N], uint64_t ex[N], bool exf[N], uint64_t tot[N], bool totf[N])
{
    __shared__ unsigned long long s_x[NT / 64][N];
    __shared__ uint32_t s_f[NT / 64][N];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t bx[N];
    uint32_t bf[N];
#pragma unroll
    for (int q = 0; q < N; ++q) {
        unsigned long long x = v[q];
        uint32_t f = head[q] ? 1u : 0u;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long y = __shfl_up(x, (unsigned)d, 64);
            const uint32_t g = __shfl_up(f, (unsigned)d, 64);
            if (lane >= d) { if (!f) x += y; f |= g; }
        }
        if (lane == 63) { s_x[wave][q] = x; s_f[wave][q] = f; }
        const unsigned long long y = __shfl_up(x, 1u, 64);
        const uint32_t g = __shfl_up(f, 1u, 64);
        bx[q] = lane ? y : 0; bf[q] = lane ? g : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < N; ++q) {
        uint64_t px = 0, ax = 0;
        uint32_t pf = 0, af = 0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) {
            const uint64_t x = s_x[w][q];
            const uint32_t f = s_f[w][q];
            if (w < wave) { px = f ? x : px + x; pf |= f; }
            ax = f ? x : ax + x; af |= f;
        }
        ex[q] = bf[q] ? bx[q] : px + bx[q];
        exf[q] = (bf[q] | pf) != 0u;
        tot[q] = ax; totf[q] = af != 0u;
    }
    __syncthreads();
}

/* one workgroup of kPlanLanes: part[8 i + q] (the sum of workgroup i's last run) and part[8 i + N + q] (non-zero: a run began in
 * it), q < N <= 4, become part[8 i + q] = the sum that the run open at workgroup i's first lane brings with it */
template <int N>
__device__ __forceinline__ void seg_scan_parts(unsigned long long* part, uint64_t blocks)
{
    static_assert(2 * N <= 8, "sums and flags share a workgroup's 8 words");
    uint64_t run[N];
#pragma unroll
    for (int q = 0; q < N; ++q) run[q] = 0;
    for (uint64_t seg = 0; seg < blocks; seg += (uint64_t)kPlanLanes * kPlanPer) {
        const uint64_t i0 = seg + (uint64_t)threadIdx.x * kPlanPer;
        uint64_t v[N] = {};
        bool f[N] = {};
        for (int i = 0; i < kPlanPer && i0 + i < blocks; ++i) {
            const unsigned long long* p = part + (i0 + i) * 8;
#pragma unroll
            for (int q = 0; q < N; ++q) {
                if (p[N + q]) { v[q] = p[q]; f[q] = true; }
                else v[q] += p[q];
            }
        }
        uint64_t ex[N], tot[N];
        bool exf[N], totf[N];
        block_seg_excl<N, kPlanLanes>(v, f, ex, exf, tot, totf);
#pragma unroll
        for (int q = 0; q < N; ++q) if (!exf[q]) ex[q] += run[q];
        for (int i = 0; i < kPlanPer && i0 + i < blocks; ++i) {
            unsigned long long* p = part + (i0 + i) * 8;
#pragma unroll
            for (int q = 0; q < N; ++q) {
                const uint64_t x = p[q];
                p[q] = ex[q];
                ex[q] = p[N + q] ? x : ex[q] + x;
            }
        }
#pragma unroll
        for (int q = 0; q < N; ++q) run[q] = totf[q] ? tot[q] : run[q] + tot[q];
    }
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
