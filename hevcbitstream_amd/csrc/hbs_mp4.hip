/*
 * hbs_mp4.hip -- hbs_mp4_fragment: the access units of an Annex-B stream -> fragmented-MP4 fragments, a moof and an mdat each,
 * the samples length-prefixed as hbs_annexb_to_lenpref makes them (include/hevcbitstream_amd.h; the bytes' rule is
 * mp4_head_word / mp4_frag_byte, hbs_mp4.h).  A plan over the NALs and one over the AUs, then a copy over 64 KiB output tiles.
 * Ten launches, none of which waits for another workgroup:
 *
 *   k_mp4_nal_count  a lane a NAL, 256 a workgroup: checks the entries, the AU numbers and the length limit;
 *                    per workgroup the sums of record bytes and kept NALs, and 1 + its lowest bad NAL
 *   k_mp4_au_count   a lane an AU, 256 a workgroup: the time rules; per workgroup 1 + its lowest bad AU and 1 + its last AU
 *                    that s() may name (AU 0, an IRAP under HBS_MP4_CUT_AT_IRAP)
 *   k_mp4_scan       one workgroup: exclusive scan of the NAL sums and exclusive maximum of the cut AUs over the workgroups
 *                    (scan_parts, max_scan_parts: hbs_plan.h); what was wrong so far
 *   k_mp4_nal_place  the NALs once more, now with the offsets: B(a) of every AU (its first NAL's lane), and with an output the
 *                    records' table: where each kept NAL's record begins among the record bytes, where its payload comes from
 *   k_mp4_frag_count the AUs once more: s(a) (block_excl_max and the maximum in front), whether a fragment begins at a; the lane
 *                    of a fragment's last AU checks its size; per workgroup the fragments that begin in it
 *   k_mp4_finish     one workgroup: exclusive scan of those counts; the totals, the error, the summary.  A plan-only call ends
 *                    here
 *   k_mp4_frag_place the AUs a third time, with the fragment numbers: the fragment of every AU; the lane of a fragment's last AU
 *                    writes where it begins, its first AU and d_frag
 *   k_mp4_samples    a lane an AU: d_sample_off / d_sample_size (only when asked for)
 *   k_mp4_tiles      a lane per 64 KiB output tile: binary search of the fragment and of the record its first byte lies in
 *   k_mp4_copy       one workgroup per output tile: the tile's fragments (at most 587: a fragment has 112 bytes or more) and
 *                    records (up to 1024; more are read from memory) are staged in LDS; each lane takes 16-byte output chunks
 *                    4 KiB apart, in the skeleton of hbs_copy16.h: copy_batches for the chunks wholly inside one NAL's payload;
 *                    the chunks that hold container bytes or a length field, or span two payloads, go to the list in LDS, and
 *                    copy_slow_list makes their bytes from the rule (chunk_byte): the byte's fragment and, in the trun array,
 *                    the one word of its sample it lies in.
 *
 * Traffic: the kept payloads read once and the output written once; the index read twice (32 B a NAL), the times, the AU flags
 * and B(a) by each AU pass and by the lanes of the trun bytes; 16 B a kept NAL, 24 B an AU and 16 B a tile of scratch.
 */
#include <hip/hip_runtime.h>
#include "hbs_mp4.h"
#include "hbs_plan.h"
#include "hbs_copy16.h"

namespace hbs {
namespace {

constexpr int kMT = kMp4Lanes;
constexpr uint32_t kTile = (uint32_t)kMp4TileBytes;
constexpr int kChunks = (int)(kMp4TileBytes / 16 / kMT);              /* 16-byte output chunks a copy lane takes  */
constexpr uint32_t kLdsRecs = 1024;                                   /* records a tile stages in LDS; more: read from memory */
constexpr uint32_t kLdsFrags = 640;                                   /* fragments a tile can hold, and two              */
static_assert(kMp4TileBytes / (kMp4FragFixed + 16) + 3 <= kLdsFrags, "every fragment of a tile is staged");
static_assert(kMp4Lanes == kPlanLanes, "the plan's workgroups share block_scan's instances with scan_parts");

enum : int { kErr = 0, kTotal = 1, kKept = 2, kFrags = 3, kBadNal = 4, kBadAu = 5, kRecBytes = 6 };      /* ctl words */

/* ---- NAL side ---------------------------------------------------------------------------------------------------------- */

struct Nal {
    uint64_t start, rec;           /* rec: record bytes (0: not kept)  */
    uint32_t raw_au;
    bool bad, kept, first_of_au;
};

/* entry k with the end of entry k-1 (0 for k = 0) and the AU word of NAL k-1: every check of the call that is about NAL k */
__device__ __forceinline__ Nal eval_nal(const Mp4Args& a, uint64_t k, uint64_t prev_end, uint32_t prev_au)
{
    const hbs_nal_entry e = a.index[k];
    Nal r;
    r.start = e.start;
    r.bad = e.start > e.end || e.end > a.n || e.start < prev_end;
    r.kept = !r.bad && (!a.keep || a.keep[k] != 0);
    if (r.kept && !mp4_len_fits(e.end - e.start, a.L)) { r.bad = true; r.kept = false; }
    r.rec = r.kept ? a.L + (e.end - e.start) : 0;
    r.raw_au = a.nal_au[k];
    r.first_of_au = k == 0 || r.raw_au != prev_au;
    if (k != 0 && r.raw_au - prev_au > 1u) r.bad = true;
    if (k == a.n_nals - 1 && (uint64_t)(r.raw_au - a.nal_au[0]) + 1 != a.n_aus) r.bad = true;
    return r;
}

__global__ __launch_bounds__(kMT) void k_mp4_nal_count(Mp4Args a)
{
    const uint64_t base = (uint64_t)blockIdx.x * kMp4NalsPerBlock + (uint64_t)threadIdx.x * kMp4NalsPer;
    uint64_t v[2] = {0, 0};
    uint64_t bad = 0;
    if (base < a.n_nals) {
        uint64_t prev = base ? a.index[base - 1].end : 0;
        uint32_t pau = base ? a.nal_au[base - 1] : 0;
        for (int i = 0; i < kMp4NalsPer && base + i < a.n_nals; ++i) {
            const Nal x = eval_nal(a, base + i, prev, pau);
            prev = a.index[base + i].end; pau = x.raw_au;
            if (x.bad && !bad) bad = base + i + 1;
            if (x.kept) { v[0] += x.rec; v[1] += 1; }
        }
    }
    bad = block_min_nonzero(bad);
    uint64_t ex[2], tot[2];
    block_scan<2, kMT>(v, ex, tot);
    if (threadIdx.x == 0) {
        unsigned long long* p = a.part_n + (uint64_t)blockIdx.x * 8;
        p[0] = tot[0]; p[1] = tot[1]; p[2] = bad;
    }
}

__global__ __launch_bounds__(kMT) void k_mp4_nal_place(Mp4Args a)
{
    if (a.ctl[kBadNal] != 0) return;
    const uint64_t base = (uint64_t)blockIdx.x * kMp4NalsPerBlock + (uint64_t)threadIdx.x * kMp4NalsPer;
    const bool in = base < a.n_nals;
    Nal x[kMp4NalsPer];                 /* the lane's entries, read once: kept in registers across the scan */
    uint64_t v[2] = {0, 0};
    uint64_t prev = (base && in) ? a.index[base - 1].end : 0;
    uint32_t pau = (base && in) ? a.nal_au[base - 1] : 0;
#pragma unroll
    for (int i = 0; i < kMp4NalsPer; ++i) {
        x[i].kept = false; x[i].first_of_au = false; x[i].rec = 0; x[i].start = 0; x[i].raw_au = 0;
        if (base + i < a.n_nals) {
            x[i] = eval_nal(a, base + i, prev, pau);
            prev = a.index[base + i].end; pau = x[i].raw_au;
            if (x[i].kept) { v[0] += x[i].rec; v[1] += 1; }
        }
    }
    uint64_t off[2], tot[2];
    block_scan<2, kMT>(v, off, tot);
    if (!in) return;
    const unsigned long long* p = a.part_n + (uint64_t)blockIdx.x * 8;
    off[0] += p[0]; off[1] += p[1];
    const uint32_t au0 = a.nal_au[0];
#pragma unroll
    for (int i = 0; i < kMp4NalsPer; ++i) {
        if (base + i >= a.n_nals) break;
        if (x[i].first_of_au) a.au_B[x[i].raw_au - au0] = off[0];         /* (the AU numbers were checked: below n_aus) */
        if (!x[i].kept) continue;
        if (a.out) {
            a.rec_B[off[1]] = off[0];
            a.rec_delta[off[1]] = x[i].start - (off[0] + a.L);
        }
        off[0] += x[i].rec; off[1] += 1;
    }
}

/* ---- AU side ----------------------------------------------------------------------------------------------------------- */

__device__ __forceinline__ bool au_dts(const Mp4Args& a, uint64_t k, uint64_t& t)
{
    if (a.dts) { t = a.dts[k]; return true; }
    return mp4_ruled_dts(a.base_time, k, a.sample_duration, t);
}

/* the time words of AU k's trun entry; false: AU k breaks a time rule */
__device__ __forceinline__ bool au_times(const Mp4Args& a, uint64_t k, uint64_t& dts, uint32_t& dur, uint32_t& cts)
{
    const bool last = k + 1 == a.n_aus;
    const bool ok = au_dts(a, k, dts);
    uint64_t next = 0;
    if (!last) {
        if (a.dts) next = a.dts[k + 1];
        else next = dts + a.sample_duration;                /* (the exact difference is sample_duration whatever wraps) */
    }
    return mp4_au_times(dts, ok, last, next, a.sample_duration, a.pts != nullptr, a.pts ? a.pts[k] : 0, dur, cts);
}

__device__ __forceinline__ bool au_cut(const Mp4Args& a, uint64_t k)
{
    return k == 0 || ((a.flags & HBS_MP4_CUT_AT_IRAP) != 0 && (a.au[k].flags & HBS_AU_IRAP) != 0);
}

__global__ __launch_bounds__(kMT) void k_mp4_au_count(Mp4Args a)
{
    const uint64_t k = (uint64_t)blockIdx.x * kMp4AusPerBlock + threadIdx.x;
    uint64_t bad = 0, cut = 0;
    if (k < a.n_aus) {
        uint64_t dts;
        uint32_t dur, cts;
        if (!au_times(a, k, dts, dur, cts)) bad = k + 1;
        if (au_cut(a, k)) cut = k + 1;
    }
    bad = block_min_nonzero(bad);
    uint64_t ex, tot;
    block_excl_max<uint64_t, 1, kMT>(&cut, &ex, &tot);
    if (threadIdx.x == 0) { a.bad_a[blockIdx.x] = bad; a.last[blockIdx.x] = tot; }
}

__global__ __launch_bounds__(kPlanLanes) void k_mp4_scan(Mp4Args a, uint64_t nal_blocks, uint64_t au_blocks)
{
    uint64_t carry[2];
    const uint64_t bad_nal = scan_parts<2>(a.part_n, nal_blocks, carry);
    (void)max_scan_parts(a.last, au_blocks);
    const uint64_t bad_au = min_nonzero_of(a.bad_a, au_blocks);
    if (threadIdx.x == 0) {
        a.ctl[kBadNal] = bad_nal; a.ctl[kBadAu] = bad_au;
        a.ctl[kRecBytes] = carry[0]; a.ctl[kKept] = carry[1];
        if (!bad_nal) {
            a.au_B[a.n_aus] = carry[0];
            if (a.out) a.rec_B[carry[1]] = carry[0];
        }
    }
}

/* where AU k stands among the fragments */
struct AuFrag {
    bool begins, ends;             /* a fragment begins at k; k is its fragment's last AU             */
    uint64_t first;                /* f_r of its fragment                                             */
};

/* cut: 1 + k when s() may name AU k, else 0; before: the maximum of that over the AUs in front of k (0: none) */
__device__ __forceinline__ AuFrag au_frag(const Mp4Args& a, uint64_t k, uint64_t cut, uint64_t before)
{
    const uint64_t s = (cut ? cut : before) - 1u;           /* (AU 0 is a cut: one of the two is non-zero) */
    const uint64_t M = a.max_samples;
    AuFrag r;
    r.first = M ? s + (k - s) / M * M : s;
    r.begins = k == r.first;
    r.ends = true;
    if (k + 1 < a.n_aus) r.ends = au_cut(a, k + 1) || (M && (k + 1 - s) % M == 0);
    return r;
}

/* the lanes' AuFrag and the fragments that begin in the workgroup's lanes in front (ex) and in all of them (tot) */
__device__ __forceinline__ AuFrag block_frags(const Mp4Args& a, uint64_t k, uint64_t& ex, uint64_t& tot)
{
    const bool in = k < a.n_aus;
    const uint64_t cut = (in && au_cut(a, k)) ? k + 1 : 0;
    uint64_t before, all;
    block_excl_max<uint64_t, 1, kMT>(&cut, &before, &all);
    const uint64_t front = a.last[blockIdx.x];
    if (front > before) before = front;
    AuFrag f;
    f.begins = false; f.ends = false; f.first = 0;
    if (in) f = au_frag(a, k, cut, before);
    const uint64_t v = f.begins ? 1 : 0;
    block_scan<1, kMT>(&v, &ex, &tot);
    return f;
}

__global__ __launch_bounds__(kMT) void k_mp4_frag_count(Mp4Args a)
{
    if (a.ctl[kBadNal] != 0) return;
    const uint64_t k = (uint64_t)blockIdx.x * kMp4AusPerBlock + threadIdx.x;
    uint64_t ex, tot;
    const AuFrag f = block_frags(a, k, ex, tot);
    uint64_t bad = 0;
    if (f.ends) {
        const uint64_t S = k + 1 - f.first, P = a.au_B[k + 1] - a.au_B[f.first];
        if (S > kMp4MaxSamples || P > kMp4MaxPayload) bad = f.first + 1;
    }
    bad = block_min_nonzero(bad);
    if (threadIdx.x == 0) {
        unsigned long long* p = a.part_a + (uint64_t)blockIdx.x * 8;
        p[0] = tot; p[1] = bad;
    }
}

__global__ __launch_bounds__(kPlanLanes) void k_mp4_finish(Mp4Args a, uint64_t au_blocks)
{
    const uint64_t bad_nal = a.ctl[kBadNal];
    uint64_t carry[1] = {0};
    uint64_t bad_au = a.ctl[kBadAu];
    if (!bad_nal) {                                          /* (else the fragments were not counted) */
        const uint64_t big = scan_parts<1>(a.part_a, au_blocks, carry);
        if (big && (!bad_au || big < bad_au)) bad_au = big;
    }
    if (threadIdx.x == 0) {
        const uint64_t R = carry[0], rec = a.ctl[kRecBytes], kept = a.ctl[kKept];
        const uint64_t total = rec + 16u * a.n_aus + (uint64_t)kMp4FragFixed * R;
        const int32_t err = (bad_nal || bad_au) ? HBS_E_ARG
                          : (a.out && (total > a.out_cap || (a.frag && R > a.frag_cap))) ? HBS_E_CAPACITY : 0;
        a.ctl[kErr] = (unsigned long long)(uint32_t)err;
        a.ctl[kTotal] = total; a.ctl[kFrags] = R;
        if (!err && a.out) { a.frag_off[R] = total; a.frag_first[R] = (uint32_t)a.n_aus; }
        hbs_summary s;
        s.nal_count = R; s.nal_found = a.n_nals; s.rbsp_bytes = rec; s.stream_bytes = total;
        s.stop_reason = 0; s.error = err;
        s.reserved[0] = bad_nal; s.reserved[1] = bad_au; s.reserved[2] = kept;
        *a.summary = s;
    }
}

__global__ __launch_bounds__(kMT) void k_mp4_frag_place(Mp4Args a)
{
    if (a.ctl[kErr] != 0) return;
    const uint64_t k = (uint64_t)blockIdx.x * kMp4AusPerBlock + threadIdx.x;
    uint64_t ex, tot;
    const AuFrag f = block_frags(a, k, ex, tot);
    if (k >= a.n_aus) return;
    const uint64_t r = a.part_a[(uint64_t)blockIdx.x * 8] + ex + (f.begins ? 1 : 0) - 1u;     /* (AU 0 begins one: never -1) */
    a.au_frag[k] = (uint32_t)r;
    if (!f.ends) return;
    const uint64_t B0 = a.au_B[f.first], O = B0 + 16u * f.first + (uint64_t)kMp4FragFixed * r;
    a.frag_off[r] = O; a.frag_first[r] = (uint32_t)f.first;
    if (a.frag) {
        hbs_mp4_frag o;
        uint64_t dts = 0;
        (void)au_dts(a, f.first, dts);
        o.out_off = O; o.out_bytes = mp4_fragment_bytes(k + 1 - f.first, a.au_B[k + 1] - B0);
        o.first_au = f.first; o.decode_time = dts;
        o.samples = (uint32_t)(k + 1 - f.first); o.sequence = a.sequence + (uint32_t)r;
        o.flags = a.au[f.first].flags & HBS_AU_IRAP; o.reserved = 0;
        a.frag[r] = o;
    }
}

__global__ __launch_bounds__(kMT) void k_mp4_samples(Mp4Args a)
{
    if (a.ctl[kErr] != 0) return;
    const uint64_t k = (uint64_t)blockIdx.x * kMT + threadIdx.x;
    if (k >= a.n_aus) return;
    const uint32_t r = a.au_frag[k];
    const uint64_t f = a.frag_first[r], S = a.frag_first[r + 1] - f, B = a.au_B[k];
    a.sample_off[k] = a.frag_off[r] + kMp4FragFixed + 16u * S + (B - a.au_B[f]);
    a.sample_size[k] = a.au_B[k + 1] - B;
}

/* ---- the copy ---------------------------------------------------------------------------------------------------------- */

__global__ __launch_bounds__(256) void k_mp4_tiles(Mp4Args a)
{
    if (a.ctl[kErr] != 0) return;
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t > a.tiles) return;
    const uint64_t total = a.ctl[kTotal], R = a.ctl[kFrags], kept = a.ctl[kKept];
    tile_first_of<kTile>(a.frag_off, R, total, t, a.tile_frag);
    const uint64_t used = (total + kTile - 1) / kTile;
    if (t > used || R == 0) return;
    uint64_t j = kept ? kept - 1 : 0;
    if (t < used && kept) {
        /* the record byte at or behind the tile's first byte */
        const uint64_t o = t * kTile;
        const uint64_t r = last_le((uint64_t)0, R - 1, o, [&](uint64_t i) { return (uint64_t)a.frag_off[i]; });
        const uint64_t f = a.frag_first[r], head = kMp4FragFixed + 16u * (a.frag_first[r + 1] - f), m = o - a.frag_off[r];
        const uint64_t p = a.au_B[f] + (m > head ? m - head : 0);
        j = last_le((uint64_t)0, kept - 1, p, [&](uint64_t i) { return (uint64_t)a.rec_B[i]; });
    }
    a.tile_rec[t] = j;
}

/* the tile's fragments [r0, r0 + fcnt) and records [j0, j0 + cnt) */
struct TileMap {
    const unsigned long long* s_foff; const uint32_t* s_ffirst; const unsigned long long* s_fpay;      /* staged: LDS */
    const unsigned long long* s_rB; const unsigned long long* s_rdelta;                                /* staged when lds */
    const unsigned long long* rec_B; const unsigned long long* rec_delta;
    uint64_t r0, j0;
    uint32_t fcnt, cnt;
    bool lds;
    __device__ __forceinline__ uint64_t foff(uint32_t i) const { return s_foff[i]; }                   /* i = fcnt: the end */
    __device__ __forceinline__ uint32_t samples(uint32_t i) const { return s_ffirst[i + 1] - s_ffirst[i]; }
    __device__ __forceinline__ uint64_t head(uint32_t i) const { return kMp4FragFixed + 16ull * samples(i); }
    /* output byte o of fragment i's mdat payload is record byte o - fpay(i) */
    __device__ __forceinline__ uint64_t fpay(uint32_t i) const { return s_fpay[i]; }
    __device__ __forceinline__ uint64_t rB(uint32_t i) const { return lds ? s_rB[i] : rec_B[j0 + i]; }   /* i = cnt: the end */
    __device__ __forceinline__ uint64_t rdelta(uint32_t i) const { return lds ? s_rdelta[i] : rec_delta[j0 + i]; }
    __device__ __forceinline__ uint32_t find_frag(uint32_t lo, uint64_t o) const
    {
        return last_le(lo, fcnt - 1, o, [&](uint32_t i) { return foff(i); });
    }
    __device__ __forceinline__ uint32_t find_rec(uint32_t lo, uint64_t p) const
    {
        return last_le(lo, cnt - 1, p, [&](uint32_t i) { return rB(i); });
    }
};

/* word w (0 duration, 1 size, 2 flags, 3 composition offset) of AU k's trun entry */
__device__ __forceinline__ uint32_t sample_word(const Mp4Args& a, uint64_t k, uint32_t w)
{
    if (w == 1u) return (uint32_t)(a.au_B[k + 1] - a.au_B[k]);
    if (w == 2u) return mp4_sample_flags((a.au[k].flags & HBS_AU_IRAP) != 0);
    uint64_t dts;
    uint32_t dur, cts;
    (void)au_times(a, k, dts, dur, cts);
    return w == 0u ? dur : cts;
}

/* output byte `cur` of a chunk that holds container bytes or a length field or spans payloads (or ends the output), from the
 * rule; fi: the fragment the chunk's first byte lies in (a fragment has 112 bytes or more: the byte lies in it or in the next) */
__device__ __forceinline__ uint32_t chunk_byte(const Mp4Args& a, const TileMap& tm, uint32_t fi, uint64_t cur)
{
    fi += cur >= tm.foff(fi + 1) ? 1u : 0u;
    const uint64_t m = cur - tm.foff(fi);
    const uint32_t S = tm.samples(fi);
    if (m < kMp4FragFixed + 16ull * S) {
        hbs_mp4_frag f;
        const uint64_t first = tm.s_ffirst[fi];
        f.out_off = tm.foff(fi); f.out_bytes = tm.foff(fi + 1) - f.out_off; f.first_au = first;
        f.samples = S; f.sequence = a.sequence + (uint32_t)(tm.r0 + fi); f.flags = 0; f.reserved = 0;
        f.decode_time = 0;
        uint32_t w, e, sw[4] = {0, 0, 0, 0};
        if (mp4_head_place(S, m, w, e)) sw[w] = sample_word(a, first + e, w);
        else if (w == 15u || w == 16u) (void)au_dts(a, first, f.decode_time);
        return mp4_frag_byte(f, a.track_id, sw, m);
    }
    const uint64_t p = cur - tm.fpay(fi);
    const uint32_t ji = tm.find_rec(0u, p);
    const uint64_t q = p - tm.rB(ji);
    if (q < a.L) return mp4_len_byte(tm.rB(ji + 1) - tm.rB(ji) - a.L, a.L, (uint32_t)q);
    return a.src[p + tm.rdelta(ji)];
}

__global__ __launch_bounds__(kMT) void k_mp4_copy(Mp4Args a)
{
    __shared__ unsigned long long s_foff[kLdsFrags + 1];
    __shared__ unsigned long long s_fpay[kLdsFrags];
    __shared__ uint32_t s_ffirst[kLdsFrags + 1];
    __shared__ unsigned long long s_rB[kLdsRecs + 1];
    __shared__ unsigned long long s_rdelta[kLdsRecs];
    __shared__ uint32_t s_slow[kTile / 16];           /* the chunks done byte by byte: chunk | its fragment's number in the tile << 12 */
    __shared__ uint32_t s_nslow;
    if (a.ctl[kErr] != 0) return;
    const uint64_t total = a.ctl[kTotal];
    const uint64_t t0 = (uint64_t)blockIdx.x * kTile;
    if (t0 >= total) return;
    const uint32_t tlen = total - t0 < kTile ? (uint32_t)(total - t0) : kTile;
    const uint64_t r0 = a.tile_frag[blockIdx.x], r1 = a.tile_frag[blockIdx.x + 1];
    const uint64_t j0 = a.tile_rec[blockIdx.x], j1 = a.tile_rec[blockIdx.x + 1];
    const uint64_t fwant = r1 - r0 + 1;               /* fragments [r0, r1]; frag_off[r1 + 1] exists (the total at the end) */
    TileMap tm;
    tm.s_foff = s_foff; tm.s_ffirst = s_ffirst; tm.s_fpay = s_fpay; tm.s_rB = s_rB; tm.s_rdelta = s_rdelta;
    tm.rec_B = a.rec_B; tm.rec_delta = a.rec_delta;
    tm.r0 = r0; tm.j0 = j0;
    tm.fcnt = fwant < kLdsFrags ? (uint32_t)fwant : kLdsFrags;            /* (never more: the static_assert above) */
    tm.cnt = (uint32_t)(j1 - j0 + 1);                 /* records [j0, j1]; rec_B[j1 + 1] exists (the total at the end) */
    tm.lds = tm.cnt <= kLdsRecs;
    for (uint32_t i = threadIdx.x; i <= tm.fcnt; i += kMT) {
        s_foff[i] = a.frag_off[r0 + i];
        s_ffirst[i] = a.frag_first[r0 + i];
        if (i < tm.fcnt) {
            const uint64_t f = a.frag_first[r0 + i], S = a.frag_first[r0 + i + 1] - f;
            s_fpay[i] = a.frag_off[r0 + i] + kMp4FragFixed + 16u * S - a.au_B[f];
        }
    }
    if (tm.lds) {
        for (uint32_t i = threadIdx.x; i <= tm.cnt; i += kMT) {
            s_rB[i] = a.rec_B[j0 + i];
            if (i < tm.cnt) s_rdelta[i] = a.rec_delta[j0 + i];
        }
    }
    if (threadIdx.x == 0) s_nslow = 0;
    __syncthreads();
    const uint32_t L = a.L;
    uint32_t flo = 0, jlo = 0;
    copy_batches<kMT, kChunks>(a.src, a.out + t0, tlen,
        [&](uint32_t r, uint32_t& fi, uint64_t& s) {
            const uint64_t o = t0 + r;
            fi = flo = tm.find_frag(flo, o);
            /* wholly in the fragment's mdat payload ... */
            if (o - tm.foff(flo) < tm.head(flo) || o + 16 > tm.foff(flo + 1)) return false;
            const uint64_t p = o - tm.fpay(flo);
            jlo = tm.find_rec(jlo, p);
            /* ... and in one record's payload */
            if (p - tm.rB(jlo) < L || p + 16 > tm.rB(jlo + 1)) return false;
            s = p + tm.rdelta(jlo);
            return true;
        },
        [&](uint32_t r, uint32_t fi) { slow_push<kTile>(s_slow, s_nslow, r, fi); });
    __syncthreads();
    copy_slow_list<kMT>(s_slow, s_nslow, a.out, t0, tlen, [&](uint32_t fi, uint64_t cur) { return chunk_byte(a, tm, fi, cur); });
}

} // namespace

hipError_t launch_mp4_fragment(const Mp4Args& a, hipStream_t st)
{
    const uint64_t nb = (a.n_nals + kMp4NalsPerBlock - 1) / kMp4NalsPerBlock, ab = (a.n_aus + kMp4AusPerBlock - 1) / kMp4AusPerBlock;
    const hipError_t e = begin_launches(a.ev_begin, st);
    if (e != hipSuccess) return e;
    if (nb) hipLaunchKernelGGL(k_mp4_nal_count, dim3((unsigned)nb), dim3(kMT), 0, st, a);
    if (ab) hipLaunchKernelGGL(k_mp4_au_count, dim3((unsigned)ab), dim3(kMT), 0, st, a);
    hipLaunchKernelGGL(k_mp4_scan, dim3(1), dim3(kPlanLanes), 0, st, a, nb, ab);
    if (nb) hipLaunchKernelGGL(k_mp4_nal_place, dim3((unsigned)nb), dim3(kMT), 0, st, a);
    if (ab) hipLaunchKernelGGL(k_mp4_frag_count, dim3((unsigned)ab), dim3(kMT), 0, st, a);
    hipLaunchKernelGGL(k_mp4_finish, dim3(1), dim3(kPlanLanes), 0, st, a, ab);
    if (a.out && nb && ab) {
        hipLaunchKernelGGL(k_mp4_frag_place, dim3((unsigned)ab), dim3(kMT), 0, st, a);
        if (a.sample_off) hipLaunchKernelGGL(k_mp4_samples, dim3((unsigned)ab), dim3(kMT), 0, st, a);
        if (a.tiles) {
            hipLaunchKernelGGL(k_mp4_tiles, dim3((unsigned)((a.tiles + 1 + 255) / 256)), dim3(256), 0, st, a);
            hipLaunchKernelGGL(k_mp4_copy, dim3((unsigned)a.tiles), dim3(kMT), 0, st, a);
        }
    }
    return end_launches(a.ev_end, st);
}

} // namespace hbs

extern "C" {

uint64_t hbs_mp4_fragment_bytes_host(uint64_t samples, uint64_t sample_bytes)
{
    return hbs::mp4_fragment_bytes(samples, sample_bytes);
}

int64_t hbs_mp4_init_host(const hbs_mp4_init_params* p, int flags, const uint8_t* const* nal, const uint64_t* nal_bytes, uint64_t n,
                          uint8_t* out, uint64_t cap)
{
    return hbs::mp4_init_host(p, flags, nal, nal_bytes, n, out, cap);
}

}
