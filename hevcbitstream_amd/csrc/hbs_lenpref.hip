/*
 * hbs_lenpref.hip -- hbs_annexb_to_lenpref and hbs_lenpref_to_annexb: Annex-B to length-prefixed NAL units (MP4 / ISOBMFF
 * samples, ISO/IEC 14496-15) and back (include/hevcbitstream_amd.h).  Both are a plan that ends in a table of "pieces" -- a
 * short literal prefix followed by a run of source bytes at its own byte misalignment -- and one copy kernel over that table.
 * Five launches each, none of which waits for another workgroup:
 *
 *   k_a2l_count / k_l2a_count   forward: one lane per 8 consecutive NALs checks the entries, the length limit and the AU
 *                    table; reverse: one lane per sample walks its chain of records.  Per workgroup the sums of output bytes
 *                    and records (forward: and kept rbsp_len), and what was wrong
 *   k_a2l_scan / k_l2a_scan     one workgroup: exclusive scan of those sums over the workgroups; totals, the error and the
 *                    summary.  A plan-only call ends here
 *   k_a2l_place / k_l2a_place   the entries / the chains once more, now with the offsets: the piece table, the output index /
 *                    the sample tables
 *   k_piece_tiles    one lane per 64 KiB output tile: binary search of the piece its first byte lies in
 *   k_piece_copy     one workgroup per output tile: each lane takes 16-byte output chunks 4 KiB apart and finds the piece of
 *                    each (the tile's pieces are staged in LDS).  A chunk inside one payload is loaded as aligned 16-byte
 *                    non-temporal loads, realigned with alignbyte and stored as one aligned 16-byte non-temporal store; a chunk
 *                    that holds a prefix byte or spans pieces, and the output's last chunk, is assembled byte by byte and
 *                    stored byte-exact.  A payload of any size spreads over the tiles it covers.
 *
 * Traffic: the payloads read once and written once; forward the index read twice (32 B a NAL) and 32 B a kept NAL of output
 * index, reverse the length fields read twice by the lane of their sample; 16 B a piece of scratch written and read, 8 B a tile.
 */
#include <hip/hip_runtime.h>
#include "hbs_lenpref.h"
#include "hbs_wave.h"

namespace hbs {
namespace {

constexpr int kLT = 256;                                              /* lanes of the plan and copy workgroups   */
constexpr int kLPer = kLenprefNalsPerBlock / kLT;                     /* NALs a forward plan lane takes          */
constexpr uint32_t kTile = (uint32_t)kLenprefTileBytes;
constexpr int kChunks = (int)(kLenprefTileBytes / 16 / kLT);          /* 16-byte output chunks a copy lane takes */
constexpr int kBatch = 4;                                             /* ... loads of that many issued together  */
constexpr uint32_t kLdsPieces = 2048;                                 /* pieces a tile stages in LDS; more: read from memory */
constexpr int32_t kFar = -8;                                          /* a piece that begins this far in front of the tile or
                                                                         further: its prefix (<= 4 bytes) is not in the tile */
static_assert(kLenprefSamplesPerBlock == kLT, "one lane per sample");

/* exclusive scan of three sums over the NT lanes of a workgroup; tot = the workgroup's totals */
template <int NT>
__device__ __forceinline__ void block_scan3(const uint64_t v[3], uint64_t ex[3], uint64_t tot[3])
{
    __shared__ unsigned long long s_w[NT / 64][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t inc[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
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
    for (int q = 0; q < 3; ++q) {
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

/* one workgroup: the per-workgroup sums part[8 i + 0..2] become their exclusive prefix sums, carry their totals; returns the
 * lowest non-zero part[8 i + 3] (0: none).  Each lane takes kLPer consecutive workgroups per step. */
__device__ __forceinline__ uint64_t scan_parts(unsigned long long* part, uint64_t blocks, uint64_t carry[3])
{
    uint64_t flag = 0;
    carry[0] = carry[1] = carry[2] = 0;
    for (uint64_t seg = 0; seg < blocks; seg += (uint64_t)kLT * kLPer) {
        const uint64_t i0 = seg + (uint64_t)threadIdx.x * kLPer;
        uint64_t v[3] = {0, 0, 0};
        for (int i = 0; i < kLPer && i0 + i < blocks; ++i) {
            const unsigned long long* p = part + (i0 + i) * 8;
            v[0] += p[0]; v[1] += p[1]; v[2] += p[2];
            if (p[3] && (!flag || p[3] < flag)) flag = p[3];
        }
        uint64_t ex[3], tot[3];
        block_scan3<kLT>(v, ex, tot);
#pragma unroll
        for (int q = 0; q < 3; ++q) ex[q] += carry[q];
        for (int i = 0; i < kLPer && i0 + i < blocks; ++i) {
            unsigned long long* p = part + (i0 + i) * 8;
            const uint64_t x0 = p[0], x1 = p[1], x2 = p[2];
            p[0] = ex[0]; p[1] = ex[1]; p[2] = ex[2];
            ex[0] += x0; ex[1] += x1; ex[2] += x2;
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) carry[q] += tot[q];
    }
    return block_min_nonzero(flag);
}

/* ---- Annex-B to length-prefixed ---------------------------------------------------------------------------------------- */

struct Nal {
    uint64_t start, end;
    uint32_t rbsp_len, au;
    int32_t status;
    bool bad, kept, first_of_au;
};

/* entry k with the end of entry k-1 (0 for k = 0) and the AU number of NAL k-1: every check of the call that is about NAL k */
__device__ __forceinline__ Nal eval_nal(const A2lArgs& a, uint64_t k, uint64_t prev_end, uint32_t prev_au)
{
    const hbs_nal_entry e = a.index[k];
    Nal r;
    r.start = e.start; r.end = e.end; r.rbsp_len = e.rbsp_len; r.status = e.status;
    r.bad = e.start > e.end || e.end > a.n || e.start < prev_end;
    r.kept = !r.bad && (!a.keep || a.keep[k] != 0);
    if (r.kept && a.t.prefix < 8 && ((e.end - e.start) >> (8u * a.t.prefix)) != 0) { r.bad = true; r.kept = false; }
    r.au = 0; r.first_of_au = false;
    if (a.nal_au) {
        r.au = a.nal_au[k];
        r.first_of_au = k == 0 || r.au != prev_au;
        if (k == 0 ? r.au != 0 : (r.au != prev_au && (uint64_t)r.au != (uint64_t)prev_au + 1)) r.bad = true;
        if (k == a.n_nals - 1 && (uint64_t)r.au + 1 != a.n_aus) r.bad = true;
    }
    return r;
}

__global__ __launch_bounds__(kLT) void k_a2l_count(A2lArgs a)
{
    const uint64_t base = (uint64_t)blockIdx.x * kLenprefNalsPerBlock + (uint64_t)threadIdx.x * kLPer;
    uint64_t v[3] = {0, 0, 0};
    bool bad = false;
    if (base < a.n_nals) {
        uint64_t prev = base ? a.index[base - 1].end : 0;
        uint32_t pau = (base && a.nal_au) ? a.nal_au[base - 1] : 0;
        for (int i = 0; i < kLPer && base + i < a.n_nals; ++i) {
            const Nal x = eval_nal(a, base + i, prev, pau);
            prev = x.end; pau = x.au;
            bad |= x.bad;
            if (x.kept) { v[0] += a.t.prefix + (x.end - x.start); v[1] += 1; v[2] += x.rbsp_len; }
        }
    }
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    uint64_t ex[3], tot[3];
    block_scan3<kLT>(v, ex, tot);
    if (threadIdx.x == 0) {
        unsigned long long* p = a.part + (uint64_t)blockIdx.x * 8;
        p[0] = tot[0]; p[1] = tot[1]; p[2] = tot[2]; p[3] = any_bad ? 1 : 0;
    }
}

__global__ __launch_bounds__(kLT) void k_a2l_scan(A2lArgs a, uint64_t blocks)
{
    uint64_t carry[3];
    const uint64_t bad = scan_parts(a.part, blocks, carry) | ((a.nal_au && !a.n_nals && a.n_aus) ? 1 : 0);
    if (threadIdx.x == 0) {
        const uint64_t total = carry[0], kept = carry[1], rbsp = carry[2];
        const int32_t err = bad ? HBS_E_ARG : (a.t.out && total > a.out_cap) ? HBS_E_CAPACITY : 0;
        a.t.ctl[0] = (unsigned long long)(uint32_t)err;
        a.t.ctl[1] = total; a.t.ctl[2] = kept;
        if (!err && a.t.out) {
            a.t.piece_out[kept] = total;
            if (a.nal_au && a.sample_off) a.sample_off[a.n_aus] = total;
        }
        hbs_summary s;
        s.nal_count = kept; s.nal_found = a.n_nals; s.rbsp_bytes = rbsp; s.stream_bytes = total;
        s.stop_reason = 0; s.error = err;
        s.reserved[0] = s.reserved[1] = s.reserved[2] = 0;
        *a.summary = s;
    }
}

__global__ __launch_bounds__(kLT) void k_a2l_place(A2lArgs a)
{
    if (a.t.ctl[0] != 0) return;
    const uint64_t base = (uint64_t)blockIdx.x * kLenprefNalsPerBlock + (uint64_t)threadIdx.x * kLPer;
    const bool in = base < a.n_nals;
    Nal x[kLPer];                       /* the lane's entries, read once: kept in registers across the scan */
    uint64_t v[3] = {0, 0, 0};
    uint64_t prev = (base && in) ? a.index[base - 1].end : 0;
    uint32_t pau = (base && in && a.nal_au) ? a.nal_au[base - 1] : 0;
#pragma unroll
    for (int i = 0; i < kLPer; ++i) {
        x[i].kept = false; x[i].first_of_au = false;
        if (base + i < a.n_nals) {
            x[i] = eval_nal(a, base + i, prev, pau);
            prev = x[i].end; pau = x[i].au;
            if (x[i].kept) { v[0] += a.t.prefix + (x[i].end - x[i].start); v[1] += 1; v[2] += x[i].rbsp_len; }
        }
    }
    uint64_t off[3], tot[3];
    block_scan3<kLT>(v, off, tot);
    if (!in) return;
    const unsigned long long* p = a.part + (uint64_t)blockIdx.x * 8;
#pragma unroll
    for (int q = 0; q < 3; ++q) off[q] += p[q];
#pragma unroll
    for (int i = 0; i < kLPer; ++i) {
        if (x[i].first_of_au && a.sample_off) a.sample_off[x[i].au] = off[0];
        if (!x[i].kept) continue;
        const uint64_t len = x[i].end - x[i].start, pay = off[0] + a.t.prefix;
        if (a.index_out) {
            hbs_nal_entry o;
            o.start = pay; o.end = pay + len;
            o.rbsp_off = off[2]; o.rbsp_len = x[i].rbsp_len;
            o.status = x[i].status & ~HBS_ST_UNTERMINATED;
            a.index_out[off[1]] = o;
        }
        a.t.piece_out[off[1]] = off[0];
        a.t.piece_delta[off[1]] = x[i].start - pay;
        off[0] = pay + len; off[1] += 1; off[2] += x[i].rbsp_len;
    }
}

/* ---- length-prefixed to Annex-B ---------------------------------------------------------------------------------------- */

/* Sample s, record by record: f(where the payload begins in the input, its length).  recs / pay: the well-formed records in
 * front of the sample's end or of what is wrong with it.  false: the sample leaves the buffer or its chain is malformed.
 * One lane walks one sample: each length field is a load that the next one's address depends on. */
template <class F>
__device__ __forceinline__ bool walk_sample(const L2aArgs& a, uint64_t s, uint64_t& recs, uint64_t& pay, F f)
{
    const uint64_t off = a.sample_off[s], size = a.sample_size[s];
    const uint32_t L = a.length_size;
    recs = 0; pay = 0;
    if (off > a.n || size > a.n - off) return false;
    uint64_t p = off;
    const uint64_t e = off + size;
#pragma unroll 1
    while (p < e) {
        if (e - p < L) return false;
        uint64_t len = 0;
        for (uint32_t b = 0; b < L; ++b) len = (len << 8) | a.t.src[p + b];
        p += L;
        if (len > e - p) return false;
        f(p, len);
        p += len; recs += 1; pay += len;
    }
    return true;
}

__global__ __launch_bounds__(kLT) void k_l2a_count(L2aArgs a)
{
    const uint64_t s = (uint64_t)blockIdx.x * kLT + threadIdx.x;
    uint64_t v[3] = {0, 0, 0};
    uint64_t bad = 0;
    if (s < a.n_samples) {
        uint64_t recs, pay;
        if (!walk_sample(a, s, recs, pay, [](uint64_t, uint64_t) {})) bad = s + 1;
        v[0] = recs * a.t.prefix + pay; v[1] = recs;
        a.samp[2 * s] = v[0]; a.samp[2 * s + 1] = recs;
    }
    bad = block_min_nonzero(bad);
    uint64_t ex[3], tot[3];
    block_scan3<kLT>(v, ex, tot);
    if (threadIdx.x == 0) {
        unsigned long long* p = a.part + (uint64_t)blockIdx.x * 8;
        p[0] = tot[0]; p[1] = tot[1]; p[2] = 0; p[3] = bad;
    }
}

__global__ __launch_bounds__(kLT) void k_l2a_scan(L2aArgs a, uint64_t blocks)
{
    uint64_t carry[3];
    const uint64_t bad = scan_parts(a.part, blocks, carry);
    if (threadIdx.x == 0) {
        const uint64_t total = carry[0], recs = carry[1];
        const int32_t err = bad ? HBS_E_ARG : (recs > a.nal_cap || (a.t.out && total > a.out_cap)) ? HBS_E_CAPACITY : 0;
        a.t.ctl[0] = (unsigned long long)(uint32_t)err;
        a.t.ctl[1] = total; a.t.ctl[2] = recs;
        if (!err && a.t.out) {
            a.t.piece_out[recs] = total;
            if (a.sample_off_out) a.sample_off_out[a.n_samples] = total;
        }
        hbs_summary s;
        s.nal_count = recs; s.nal_found = a.n_samples; s.rbsp_bytes = 0; s.stream_bytes = total;
        s.stop_reason = recs ? -1 : 0; s.error = err;
        s.reserved[0] = bad; s.reserved[1] = s.reserved[2] = 0;
        *a.summary = s;
    }
}

__global__ __launch_bounds__(kLT) void k_l2a_place(L2aArgs a)
{
    if (a.t.ctl[0] != 0) return;
    const uint64_t s = (uint64_t)blockIdx.x * kLT + threadIdx.x;
    const bool in = s < a.n_samples;
    uint64_t v[3] = {0, 0, 0};
    if (in) { v[0] = a.samp[2 * s]; v[1] = a.samp[2 * s + 1]; }
    uint64_t off[3], tot[3];
    block_scan3<kLT>(v, off, tot);
    if (!in) return;
    const unsigned long long* p = a.part + (uint64_t)blockIdx.x * 8;
    uint64_t o = off[0] + p[0], r = off[1] + p[1];
    if (a.sample_off_out) a.sample_off_out[s] = o;
    const uint32_t sc = a.t.prefix;
    unsigned long long* const piece_out = a.t.piece_out;
    unsigned long long* const piece_delta = a.t.piece_delta;
    uint64_t recs, pay;
    (void)walk_sample(a, s, recs, pay, [&](uint64_t src, uint64_t len) {
        piece_out[r] = o;
        piece_delta[r] = src - (o + sc);
        o += sc + len; r += 1;
    });
}

/* ---- the copy over the piece table ------------------------------------------------------------------------------------- */

__global__ __launch_bounds__(256) void k_piece_tiles(PieceTable a)
{
    if (a.ctl[0] != 0) return;
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t total = a.ctl[1], pieces = a.ctl[2];
    const uint64_t used = (total + kTile - 1) / kTile;
    if (t > used || pieces == 0) return;
    if (t == used) { a.tile_first[t] = pieces - 1; return; }
    const uint64_t o = t * kTile;
    uint64_t lo = 0, hi = pieces - 1;                /* the last piece that begins at or before o */
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (a.piece_out[mid] <= o) lo = mid; else hi = mid - 1;
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

/* the tile's pieces [j0, j0 + cnt): rel(i) = where piece j0 + i begins, relative to the tile (clamped to [kFar, kTile]) */
struct TilePieces {
    const int32_t* s_bound; const unsigned long long* s_delta;     /* staged: LDS */
    const unsigned long long* piece_out; const unsigned long long* piece_delta;
    uint64_t j0, t0;
    bool lds;
    __device__ __forceinline__ int32_t rel(uint32_t i) const
    {
        if (lds) return s_bound[i];
        const uint64_t b = piece_out[j0 + i];
        if (b >= t0) return b - t0 >= kTile ? (int32_t)kTile : (int32_t)(b - t0);
        return t0 - b >= (uint64_t)(-kFar) ? kFar : -(int32_t)(t0 - b);
    }
    __device__ __forceinline__ uint64_t delta(uint32_t i) const { return lds ? s_delta[i] : piece_delta[j0 + i]; }
    /* the last piece i in [lo, hi] with rel(i) <= r (rel(lo) <= r holds) */
    __device__ __forceinline__ uint32_t find(uint32_t lo, uint32_t hi, uint32_t r) const
    {
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (rel(mid) <= (int32_t)r) lo = mid; else hi = mid - 1;
        }
        return lo;
    }
};

/* an output chunk [r, r + len) of the tile that holds prefix bytes or spans pieces (or ends the output): assembled byte by
 * byte, each payload byte loaded from the piece it belongs to, each prefix byte computed */
__device__ __forceinline__ void copy_chunk_bytes(const PieceTable& a, const TilePieces& tp, uint32_t ip, uint32_t r, uint32_t len)
{
    uint64_t clo = 0, chi = 0;
    int32_t b0 = tp.rel(ip), b1 = tp.rel(ip + 1);
    uint64_t delta = tp.delta(ip);
    uint64_t plen = 0;
    bool have_len = false;
    const int32_t P = (int32_t)a.prefix;
#pragma unroll 1
    for (uint32_t q = 0; q < len; ++q) {
        const int32_t ro = (int32_t)(r + q);
        if (ro >= b1) { ip += 1; b0 = b1; b1 = tp.rel(ip + 1); delta = tp.delta(ip); have_len = false; }
        const int32_t pos = ro - b0;           /* (a piece clamped to kFar: pos >= 8, payload) */
        uint64_t v;
        if (pos >= P) {
            v = a.src[delta + tp.t0 + (uint32_t)ro];
        } else if (a.prefix_is_length) {
            if (!have_len) { plen = a.piece_out[tp.j0 + ip + 1] - a.piece_out[tp.j0 + ip] - (uint64_t)P; have_len = true; }
            v = (plen >> (8 * (P - 1 - pos))) & 0xFFu;
        } else {
            v = pos == P - 1 ? 1u : 0u;
        }
        if (q < 8) clo |= v << (8 * q); else chi |= v << (8 * (q - 8));
    }
    uint8_t* dst = a.out + tp.t0 + r;
    if (len == 16) {
        u32x4 c;
        c.x = (uint32_t)clo; c.y = (uint32_t)(clo >> 32); c.z = (uint32_t)chi; c.w = (uint32_t)(chi >> 32);
        arena_store16(dst, c);
    } else {
        store_pieces(dst, clo, chi, len);
    }
}

__global__ __launch_bounds__(kLT) void k_piece_copy(PieceTable a)
{
    __shared__ int32_t s_bound[kLdsPieces + 1];
    __shared__ unsigned long long s_delta[kLdsPieces];
    if (a.ctl[0] != 0) return;
    const uint64_t total = a.ctl[1];
    const uint64_t t0 = (uint64_t)blockIdx.x * kTile;
    if (t0 >= total) return;
    const uint32_t tlen = total - t0 < kTile ? (uint32_t)(total - t0) : kTile;
    const uint64_t j0 = a.tile_first[blockIdx.x], j1 = a.tile_first[blockIdx.x + 1];
    const uint32_t cnt = (uint32_t)(j1 - j0 + 1);     /* pieces [j0, j1]; piece_out[j1 + 1] exists (the total at the end) */
    TilePieces tp;
    tp.s_bound = s_bound; tp.s_delta = s_delta; tp.piece_out = a.piece_out; tp.piece_delta = a.piece_delta;
    tp.j0 = j0; tp.t0 = t0; tp.lds = false;
    if (cnt <= kLdsPieces) {
        for (uint32_t i = threadIdx.x; i <= cnt; i += kLT) {
            s_bound[i] = tp.rel(i);
            if (i < cnt) s_delta[i] = a.piece_delta[j0 + i];
        }
        __syncthreads();
        tp.lds = true;
    }
    const int32_t P = (int32_t)a.prefix;
    uint32_t lo = 0;
    uint32_t slow = 0;                        /* chunks done byte by byte, behind the batches: bit b + u */
    uint32_t slow_ip[kChunks];
#pragma unroll 1
    for (int b = 0; b < kChunks; b += kBatch) {
        u32x4 va[kBatch], vb[kBatch];
        uint32_t sh[kBatch], ip[kBatch];
        bool simple[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const uint32_t r = 16u * (threadIdx.x + (uint32_t)kLT * (uint32_t)(b + u));
            simple[u] = false; sh[u] = 0; ip[u] = lo;
            va[u] = zero4(); vb[u] = zero4();
            if (r < tlen) {
                lo = tp.find(lo, cnt - 1, r);
                ip[u] = lo;
                if (tlen - r >= 16 && tp.rel(lo + 1) - (int32_t)r >= 16 && (int32_t)r - tp.rel(lo) >= P) {
                    const uint64_t s = tp.delta(lo) + t0 + r;
                    const uint64_t g = s & ~15ull;
                    sh[u] = (uint32_t)(s & 15u);
                    simple[u] = true;
                    va[u] = stream_load16(reinterpret_cast<const u32x4*>(a.src + g));
                    if (sh[u]) vb[u] = stream_load16(reinterpret_cast<const u32x4*>(a.src + g + 16));
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const uint32_t r = 16u * (threadIdx.x + (uint32_t)kLT * (uint32_t)(b + u));
            if (simple[u]) arena_store16(a.out + t0 + r, realign(va[u], vb[u], sh[u]));
            else if (r < tlen) { slow |= 1u << (b + u); slow_ip[b + u] = ip[u]; }
        }
    }
#pragma unroll 1
    while (slow) {
        const int i = (int)__builtin_ctz(slow);
        slow &= slow - 1;
        const uint32_t r = 16u * (threadIdx.x + (uint32_t)kLT * (uint32_t)i);
        copy_chunk_bytes(a, tp, slow_ip[i], r, tlen - r < 16 ? tlen - r : 16u);
    }
}

hipError_t copy_pieces(const PieceTable& t, hipStream_t st)
{
    if (!t.tiles) return hipSuccess;
    hipLaunchKernelGGL(k_piece_tiles, dim3((unsigned)((t.tiles + 1 + 255) / 256)), dim3(256), 0, st, t);
    hipLaunchKernelGGL(k_piece_copy, dim3((unsigned)t.tiles), dim3(kLT), 0, st, t);
    return hipSuccess;
}

} // namespace

hipError_t launch_annexb_to_lenpref(const A2lArgs& a, hipStream_t st)
{
    const uint64_t blocks = (a.n_nals + kLenprefNalsPerBlock - 1) / kLenprefNalsPerBlock;
    hipError_t e = hipSuccess;
    if (a.ev_begin) { e = hipEventRecord(a.ev_begin, st); if (e != hipSuccess) return e; }
    if (blocks) hipLaunchKernelGGL(k_a2l_count, dim3((unsigned)blocks), dim3(kLT), 0, st, a);
    hipLaunchKernelGGL(k_a2l_scan, dim3(1), dim3(kLT), 0, st, a, blocks);
    if (a.t.out && blocks) {
        hipLaunchKernelGGL(k_a2l_place, dim3((unsigned)blocks), dim3(kLT), 0, st, a);
        (void)copy_pieces(a.t, st);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (a.ev_end) e = hipEventRecord(a.ev_end, st);
    return e;
}

hipError_t launch_lenpref_to_annexb(const L2aArgs& a, hipStream_t st)
{
    const uint64_t blocks = (a.n_samples + kLenprefSamplesPerBlock - 1) / kLenprefSamplesPerBlock;
    hipError_t e = hipSuccess;
    if (a.ev_begin) { e = hipEventRecord(a.ev_begin, st); if (e != hipSuccess) return e; }
    if (blocks) hipLaunchKernelGGL(k_l2a_count, dim3((unsigned)blocks), dim3(kLT), 0, st, a);
    hipLaunchKernelGGL(k_l2a_scan, dim3(1), dim3(kLT), 0, st, a, blocks);
    if (a.t.out && blocks) {
        hipLaunchKernelGGL(k_l2a_place, dim3((unsigned)blocks), dim3(kLT), 0, st, a);
        (void)copy_pieces(a.t, st);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (a.ev_end) e = hipEventRecord(a.ev_end, st);
    return e;
}

} // namespace hbs
