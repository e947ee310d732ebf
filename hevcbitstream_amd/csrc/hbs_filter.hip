/*
 * hbs_filter.hip -- hbs_filter_annexb: cut an Annex-B stream down to some of its NAL units
 * (include/hevcbitstream_amd.h).  Five launches, none of which waits for another workgroup:
 *
 *   k_filter_count   one lane per 8 consecutive NALs: check the entry, read its two header bytes, apply the
 *                    rule (or d_keep); per workgroup of 2048 NALs the sums of kept unit bytes, kept NALs, kept
 *                    rbsp_len, kept non-empty units, and whether an entry was inconsistent
 *   k_filter_scan    one workgroup: exclusive scan of those sums over the workgroups; totals, the error
 *                    (HBS_E_ARG, HBS_E_CAPACITY against out_cap) and the summary
 *   k_filter_place   the count again, now with the workgroup's offsets: the output index, and per kept non-empty
 *                    unit its output offset and its stream offset (minus the output offset), in kept order
 *   k_filter_tiles   one lane per 64 KiB output tile: binary search of the unit its first byte lies in
 *   k_filter_copy    one workgroup per output tile: each lane takes 16-byte output chunks 4 KiB apart, finds the
 *                    unit of each (the tile's units are staged in LDS), loads the source as aligned 16-byte
 *                    non-temporal loads, realigns them with alignbyte and writes aligned 16-byte non-temporal
 *                    stores; a chunk that spans units is assembled byte by byte, the output's last chunk is
 *                    stored byte-exact.  A unit of any size spreads over the tiles it covers.
 *
 * Traffic: the kept units read once and written once, the index read twice (32 B a NAL, count and place), 32 B a
 * kept NAL of output index, 16 B a kept unit of scratch written and read, 8 B a tile.
 */
#include <hip/hip_runtime.h>
#include "hbs_filter.h"
#include "hbs_wave.h"

namespace hbs {
namespace {

constexpr int kFT = 256;                                              /* lanes of the plan and copy workgroups */
constexpr int kFPer = kFilterNalsPerBlock / kFT;                      /* NALs a plan lane takes                */
constexpr uint32_t kTile = (uint32_t)kFilterTileBytes;
constexpr int kChunks = (int)(kFilterTileBytes / 16 / kFT);           /* 16-byte output chunks a copy lane takes */
constexpr int kBatch = 4;                                             /* ... loads of that many issued together  */
constexpr uint32_t kLdsUnits = 2048;                                  /* units a tile stages in LDS; more: read from memory */

struct Nal {
    uint64_t u, start, end;      /* unit [u, end); payload [start, end) */
    uint32_t rbsp_len;
    int32_t status;
    bool bad, kept;
};

/* entry k with the end of entry k-1 (0 for k = 0): checked before its header bytes are read */
__device__ __forceinline__ Nal eval_nal(const FilterArgs& a, uint64_t k, uint64_t prev_end)
{
    const hbs_nal_entry e = a.index[k];
    Nal r;
    r.u = prev_end; r.start = e.start; r.end = e.end; r.rbsp_len = e.rbsp_len; r.status = e.status;
    r.bad = e.start > e.end || e.end > a.n || e.start < prev_end;
    bool keep = false;
    if (!r.bad) {
        if (!a.use_rule) {
            keep = a.keep[k] != 0;
        } else if (e.end - e.start < 2) {
            keep = a.rule.keep_short != 0;
        } else {
            const uint32_t b0 = a.stream[e.start], b1 = a.stream[e.start + 1];
            const uint32_t type = (b0 >> 1) & 63u;
            const int32_t layer = (int32_t)(((b0 & 1u) << 5) | (b1 >> 3));
            const int32_t tid1 = (int32_t)(b1 & 7u);
            keep = ((a.rule.keep_types >> type) & 1ull) && tid1 <= a.rule.max_temporal_id_plus1 && layer <= a.rule.max_layer_id;
        }
    }
    r.kept = keep;
    return r;
}

/* exclusive scan of four sums over the NT lanes of a workgroup; tot = the workgroup's totals */
template <int NT>
__device__ __forceinline__ void block_scan4(const uint64_t v[4], uint64_t ex[4], uint64_t tot[4])
{
    __shared__ unsigned long long s_w[NT / 64][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t inc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
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
    for (int q = 0; q < 4; ++q) {
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

__global__ __launch_bounds__(kFT) void k_filter_count(FilterArgs a)
{
    const uint64_t base = (uint64_t)blockIdx.x * kFilterNalsPerBlock + (uint64_t)threadIdx.x * kFPer;
    uint64_t v[4] = {0, 0, 0, 0};
    bool bad = false;
    if (base < a.n_nals) {
        uint64_t prev = base ? a.index[base - 1].end : 0;
        for (int i = 0; i < kFPer && base + i < a.n_nals; ++i) {
            const Nal x = eval_nal(a, base + i, prev);
            prev = x.end;
            bad |= x.bad;
            if (x.kept) {
                const uint64_t unit = x.end - x.u;
                v[0] += unit; v[1] += 1; v[2] += x.rbsp_len; v[3] += unit ? 1 : 0;
            }
        }
    }
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    uint64_t ex[4], tot[4];
    block_scan4<kFT>(v, ex, tot);
    if (threadIdx.x == 0) {
        unsigned long long* p = a.part + (uint64_t)blockIdx.x * 8;
        p[0] = tot[0]; p[1] = tot[1]; p[2] = tot[2]; p[3] = tot[3]; p[4] = any_bad ? 1 : 0;
    }
}

/* one workgroup; each lane takes kFPer consecutive workgroup sums per step of kFilterNalsPerBlock of them */
__global__ __launch_bounds__(kFT) void k_filter_scan(FilterArgs a, uint64_t blocks)
{
    uint64_t carry[4] = {0, 0, 0, 0};
    int bad = 0;
    for (uint64_t seg = 0; seg < blocks; seg += kFilterNalsPerBlock) {
        const uint64_t i0 = seg + (uint64_t)threadIdx.x * kFPer;
        uint64_t v[4] = {0, 0, 0, 0};
        for (int i = 0; i < kFPer && i0 + i < blocks; ++i) {
            const unsigned long long* p = a.part + (i0 + i) * 8;
            v[0] += p[0]; v[1] += p[1]; v[2] += p[2]; v[3] += p[3];
            bad |= p[4] != 0;
        }
        uint64_t ex[4], tot[4];
        block_scan4<kFT>(v, ex, tot);
#pragma unroll
        for (int q = 0; q < 4; ++q) ex[q] += carry[q];
        for (int i = 0; i < kFPer && i0 + i < blocks; ++i) {
            unsigned long long* p = a.part + (i0 + i) * 8;
            const uint64_t x0 = p[0], x1 = p[1], x2 = p[2], x3 = p[3];
            p[0] = ex[0]; p[1] = ex[1]; p[2] = ex[2]; p[3] = ex[3];
            ex[0] += x0; ex[1] += x1; ex[2] += x2; ex[3] += x3;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) carry[q] += tot[q];
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
        const uint64_t total = carry[0], kept = carry[1], rbsp = carry[2], units = carry[3];
        const int32_t err = bad ? HBS_E_ARG : (a.out && total > a.out_cap) ? HBS_E_CAPACITY : 0;
        a.ctl[0] = (unsigned long long)(uint32_t)err;
        a.ctl[1] = total; a.ctl[2] = units; a.ctl[3] = kept;
        if (!err && a.out) a.kept_out[units] = total;
        hbs_summary s;
        s.nal_count = kept; s.nal_found = a.n_nals; s.rbsp_bytes = rbsp; s.stream_bytes = total;
        s.stop_reason = kept ? -1 : 0; s.error = err;
        s.reserved[0] = s.reserved[1] = s.reserved[2] = 0;
        *a.summary = s;
    }
}

__global__ __launch_bounds__(kFT) void k_filter_place(FilterArgs a)
{
    if (a.ctl[0] != 0) return;
    const uint64_t base = (uint64_t)blockIdx.x * kFilterNalsPerBlock + (uint64_t)threadIdx.x * kFPer;
    const uint64_t prev0 = (base && base < a.n_nals) ? a.index[base - 1].end : 0;
    uint64_t v[4] = {0, 0, 0, 0};
    if (base < a.n_nals) {
        uint64_t prev = prev0;
        for (int i = 0; i < kFPer && base + i < a.n_nals; ++i) {
            const Nal x = eval_nal(a, base + i, prev);
            prev = x.end;
            if (x.kept) {
                const uint64_t unit = x.end - x.u;
                v[0] += unit; v[1] += 1; v[2] += x.rbsp_len; v[3] += unit ? 1 : 0;
            }
        }
    }
    uint64_t off[4], tot[4];
    block_scan4<kFT>(v, off, tot);
    if (base >= a.n_nals) return;
    const unsigned long long* p = a.part + (uint64_t)blockIdx.x * 8;
#pragma unroll
    for (int q = 0; q < 4; ++q) off[q] += p[q];
    const uint64_t last = a.ctl[3] - 1;          /* rank of the last kept NAL */
    uint64_t prev = prev0;
    for (int i = 0; i < kFPer && base + i < a.n_nals; ++i) {
        const Nal x = eval_nal(a, base + i, prev);
        prev = x.end;
        if (!x.kept) continue;
        const uint64_t unit = x.end - x.u;
        if (a.index_out) {
            hbs_nal_entry o;
            o.start = off[0] + (x.start - x.u);
            o.end = off[0] + unit;
            o.rbsp_off = off[2];
            o.rbsp_len = x.rbsp_len;
            o.status = (x.status & ~HBS_ST_UNTERMINATED) | (off[1] == last ? HBS_ST_UNTERMINATED : 0);
            a.index_out[off[1]] = o;
        }
        if (unit) {
            a.kept_out[off[3]] = off[0];
            a.kept_delta[off[3]] = x.u - off[0];
            off[3] += 1;
        }
        off[0] += unit; off[1] += 1; off[2] += x.rbsp_len;
    }
}

__global__ __launch_bounds__(256) void k_filter_tiles(FilterArgs a)
{
    if (a.ctl[0] != 0) return;
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t total = a.ctl[1], units = a.ctl[2];
    const uint64_t used = (total + kTile - 1) / kTile;
    if (t > used || units == 0) return;
    if (t == used) { a.tile_first[t] = units - 1; return; }
    const uint64_t o = t * kTile;
    uint64_t lo = 0, hi = units - 1;                 /* the last unit that begins at or before o */
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (a.kept_out[mid] <= o) lo = mid; else hi = mid - 1;
    }
    a.tile_first[t] = lo;
}

/* bytes [sh, sh + 16) of the 32 bytes a:b */
__device__ __forceinline__ u32x4 realign(u32x4 a, u32x4 b, uint32_t sh)
{
    const uint32_t q = sh >> 2, r = sh & 3u;
    uint32_t x0, x1, x2, x3, x4;
    if (q == 0)      { x0 = a.x; x1 = a.y; x2 = a.z; x3 = a.w; x4 = b.x; }
    else if (q == 1) { x0 = a.y; x1 = a.z; x2 = a.w; x3 = b.x; x4 = b.y; }
    else if (q == 2) { x0 = a.z; x1 = a.w; x2 = b.x; x3 = b.y; x4 = b.z; }
    else             { x0 = a.w; x1 = b.x; x2 = b.y; x3 = b.z; x4 = b.w; }
    u32x4 v;
    v.x = alignbyte(x1, x0, r); v.y = alignbyte(x2, x1, r); v.z = alignbyte(x3, x2, r); v.w = alignbyte(x4, x3, r);
    return v;
}

__device__ __forceinline__ u32x4 zero4() { u32x4 z; z.x = z.y = z.z = z.w = 0; return z; }




/* the tile's units [j0, j0 + cnt): rel(i) = where unit j0 + i begins, relative to the tile (clamped to [0, kTile]) */
struct TileUnits {
    const uint32_t* s_bound; const unsigned long long* s_delta;     /* staged: LDS */
    const unsigned long long* kept_out; const unsigned long long* kept_delta;
    uint64_t j0, t0;
    bool lds;
    __device__ __forceinline__ uint32_t rel(uint32_t i) const
    {
        if (lds) return s_bound[i];
        const uint64_t b = kept_out[j0 + i];
        return b <= t0 ? 0u : (b - t0 >= kTile ? kTile : (uint32_t)(b - t0));
    }
    __device__ __forceinline__ uint64_t delta(uint32_t i) const { return lds ? s_delta[i] : kept_delta[j0 + i]; }
    /* the last unit i in [lo, hi] with rel(i) <= r (rel(lo) <= r holds) */
    __device__ __forceinline__ uint32_t find(uint32_t lo, uint32_t hi, uint32_t r) const
    {
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (rel(mid) <= r) lo = mid; else hi = mid - 1;
        }
        return lo;
    }
};

/* an output chunk [r, r + len) of the tile that spans units (or ends the output): assembled byte by byte, each byte loaded
 * from the unit it belongs to */
__device__ __forceinline__ void copy_chunk_pieces(const FilterArgs& a, const TileUnits& tu, uint32_t iu, uint32_t r, uint32_t len)
{
    uint64_t clo = 0, chi = 0;
    uint32_t b1 = tu.rel(iu + 1);
    uint64_t delta = tu.delta(iu);
#pragma unroll 1
    for (uint32_t q = 0; q < len; ++q) {
        const uint32_t ro = r + q;
        if (ro >= b1) { iu += 1; b1 = tu.rel(iu + 1); delta = tu.delta(iu); }
        const uint64_t v = a.stream[delta + tu.t0 + ro];
        if (q < 8) clo |= v << (8 * q); else chi |= v << (8 * (q - 8));
    }
    uint8_t* dst = a.out + tu.t0 + r;
    if (len == 16) {
        u32x4 c;
        c.x = (uint32_t)clo; c.y = (uint32_t)(clo >> 32); c.z = (uint32_t)chi; c.w = (uint32_t)(chi >> 32);
        arena_store16(dst, c);
    } else {
        store_pieces(dst, clo, chi, len);
    }
}

__global__ __launch_bounds__(kFT) void k_filter_copy(FilterArgs a)
{
    __shared__ uint32_t s_bound[kLdsUnits + 1];
    __shared__ unsigned long long s_delta[kLdsUnits];
    if (a.ctl[0] != 0) return;
    const uint64_t total = a.ctl[1];
    const uint64_t t0 = (uint64_t)blockIdx.x * kTile;
    if (t0 >= total) return;
    const uint32_t tlen = total - t0 < kTile ? (uint32_t)(total - t0) : kTile;
    const uint64_t j0 = a.tile_first[blockIdx.x], j1 = a.tile_first[blockIdx.x + 1];
    const uint32_t cnt = (uint32_t)(j1 - j0 + 1);     /* units [j0, j1]; kept_out[j1 + 1] exists (the total at the end) */
    TileUnits tu;
    tu.s_bound = s_bound; tu.s_delta = s_delta; tu.kept_out = a.kept_out; tu.kept_delta = a.kept_delta;
    tu.j0 = j0; tu.t0 = t0; tu.lds = false;
    if (cnt <= kLdsUnits) {
        for (uint32_t i = threadIdx.x; i <= cnt; i += kFT) {
            s_bound[i] = tu.rel(i);
            if (i < cnt) s_delta[i] = a.kept_delta[j0 + i];
        }
        __syncthreads();
        tu.lds = true;
    }
    uint32_t lo = 0;
    uint32_t pieces = 0;                      /* chunks that span units or end the output: bit b + u, done behind the batches */
    uint32_t piece_iu[kChunks];
#pragma unroll 1
    for (int b = 0; b < kChunks; b += kBatch) {
        u32x4 va[kBatch], vb[kBatch];
        uint32_t sh[kBatch], iu[kBatch];
        bool simple[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const uint32_t r = 16u * (threadIdx.x + (uint32_t)kFT * (uint32_t)(b + u));
            simple[u] = false; sh[u] = 0; iu[u] = lo;
            va[u] = zero4(); vb[u] = zero4();
            if (r < tlen) {
                lo = tu.find(lo, cnt - 1, r);
                iu[u] = lo;
                if (tlen - r >= 16 && tu.rel(lo + 1) - r >= 16) {
                    const uint64_t s = tu.delta(lo) + t0 + r;
                    const uint64_t g = s & ~15ull;
                    sh[u] = (uint32_t)(s & 15u);
                    simple[u] = true;
                    va[u] = stream_load16(reinterpret_cast<const u32x4*>(a.stream + g));
                    if (sh[u]) vb[u] = stream_load16(reinterpret_cast<const u32x4*>(a.stream + g + 16));
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const uint32_t r = 16u * (threadIdx.x + (uint32_t)kFT * (uint32_t)(b + u));
            if (simple[u]) arena_store16(a.out + t0 + r, realign(va[u], vb[u], sh[u]));
            else if (r < tlen) { pieces |= 1u << (b + u); piece_iu[b + u] = iu[u]; }
        }
    }
#pragma unroll 1
    while (pieces) {
        const int i = (int)__builtin_ctz(pieces);
        pieces &= pieces - 1;
        const uint32_t r = 16u * (threadIdx.x + (uint32_t)kFT * (uint32_t)i);
        copy_chunk_pieces(a, tu, piece_iu[i], r, tlen - r < 16 ? tlen - r : 16u);
    }
}

} // namespace

hipError_t launch_filter_annexb(const FilterArgs& a, hipStream_t st)
{
    const uint64_t blocks = (a.n_nals + kFilterNalsPerBlock - 1) / kFilterNalsPerBlock;
    hipError_t e = hipSuccess;
    if (a.ev_begin) { e = hipEventRecord(a.ev_begin, st); if (e != hipSuccess) return e; }
    if (blocks) hipLaunchKernelGGL(k_filter_count, dim3((unsigned)blocks), dim3(kFT), 0, st, a);
    hipLaunchKernelGGL(k_filter_scan, dim3(1), dim3(kFT), 0, st, a, blocks);
    if (a.out && blocks) {
        hipLaunchKernelGGL(k_filter_place, dim3((unsigned)blocks), dim3(kFT), 0, st, a);
        if (a.tiles) {
            hipLaunchKernelGGL(k_filter_tiles, dim3((unsigned)((a.tiles + 1 + 255) / 256)), dim3(256), 0, st, a);
            hipLaunchKernelGGL(k_filter_copy, dim3((unsigned)a.tiles), dim3(kFT), 0, st, a);
        }
    }
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (a.ev_end) e = hipEventRecord(a.ev_end, st);
    return e;
}

} // namespace hbs
