/*
 * hbs_copy16.h -- device-only, for .hip files: what the copies that take one lane per aligned 16-byte output chunk share
 * (hbs_pieces.hip, hbs_rtp.hip, hbs_tsmux.hip, hbs_ts.hip, hbs_mp4.hip, hbs_mp4prot.hip).  The fast path of a chunk that lies inside one run of source bytes:
 * load16_pair, realign, arena_store16 (hbs_wave.h).  The slow path of a chunk that holds other bytes or spans runs: pack_byte
 * for each byte, then store_chunk.  last_le finds the unit a chunk lies in, tile_first_of the unit an output tile begins in.
 *
 * The skeleton around them, the same in k_piece_copy, k_rtp_copy, k_tsm_copy, k_mp4_copy and k_prot_copy, has two phases:
 *
 *   copy_batches    each lane walks its 16-byte output chunks, kLanes chunks apart, kBatch at a time.  In the first half of a
 *                   batch the kernel's locate() says for each chunk whether it lies wholly inside one run of source bytes, and
 *                   such a chunk issues load16_pair: kBatch chunks' loads are in flight a lane.  The second half realigns and
 *                   stores them, and hands every other chunk of the range to the kernel's defer().  k_rtp_copy, k_mp4_copy and
 *                   k_prot_copy call it; k_piece_copy and k_tsm_copy keep the loop written out, each with a row that ran
 *                   longer with the call (profiles/r26/copy_time.txt)
 *   the slow chunks behind the batches, byte by byte from the kernel's own rule.  Either they were noted in registers (a bit
 *                   mask: k_piece_copy, k_tsm_copy) and the lane that met a chunk assembles it, or defer() put them on a list
 *                   in LDS (slow_push) and copy_slow_list spreads the tile's list over the workgroup, a lane a byte
 */
#ifndef HBS_COPY16_H
#define HBS_COPY16_H

#include "hbs_wave.h"

namespace hbs {

__device__ __forceinline__ u32x4 zero4() { u32x4 z; z.x = z.y = z.z = z.w = 0; return z; }

/* bytes [r, r + 16) of the 20 bytes x0 .. x4; r in 0..3 */
__device__ __forceinline__ u32x4 align5(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3, uint32_t x4, uint32_t r)
{
    u32x4 v;
    v.x = alignbyte(x1, x0, r); v.y = alignbyte(x2, x1, r); v.z = alignbyte(x3, x2, r); v.w = alignbyte(x4, x3, r);
    return v;
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
    return align5(x0, x1, x2, x3, x4, r);
}

/* bytes [r, r + 16) of the five dwords at d (an image in LDS); r in 0..3 */
__device__ __forceinline__ u32x4 realign(const uint32_t* d, uint32_t r)
{
    const uint32_t x0 = d[0], x1 = d[1], x2 = d[2], x3 = d[3], x4 = d[4];
    return align5(x0, x1, x2, x3, x4, r);
}

/* the fast path's loads for the 16 bytes at src + s: the aligned 16 bytes that hold the first, non-temporal, and the next 16
 * only when s is not aligned (vb is left as it is otherwise); realign(va, vb, sh) is the 16 bytes */
__device__ __forceinline__ void load16_pair(const uint8_t* src, uint64_t s, u32x4& va, u32x4& vb, uint32_t& sh)
{
    const uint64_t g = s & ~15ull;
    sh = (uint32_t)(s & 15u);
    va = stream_load16(reinterpret_cast<const u32x4*>(src + g));
    if (sh) vb = stream_load16(reinterpret_cast<const u32x4*>(src + g + 16));
}

/* the slow path: byte q (0..15) of the chunk clo:chi becomes v (the chunk starts as zeros) */
__device__ __forceinline__ void pack_byte(uint64_t& clo, uint64_t& chi, uint32_t q, uint64_t v)
{
    if (q < 8) clo |= v << (8 * q); else chi |= v << (8 * (q - 8));
}

/* ... and its end: a whole chunk is one aligned 16-byte non-temporal store; of a partial one (an end of the output or of a
 * round's range) these `len` bytes are stored and no others */
__device__ __forceinline__ void store_chunk(uint8_t* dst, uint64_t clo, uint64_t chi, uint32_t len)
{
    if (len == 16u) {
        u32x4 c;
        c.x = (uint32_t)clo; c.y = (uint32_t)(clo >> 32); c.z = (uint32_t)chi; c.w = (uint32_t)(chi >> 32);
        arena_store16(dst, c);
    } else {
        store_pieces(dst, clo, chi, len);
    }
}

/* the last i in [lo, hi] with at(i) <= key, for a non-decreasing at() with at(lo) <= key (lo itself is never asked) */
template <class I, class K, class At>
__device__ __forceinline__ I last_le(I lo, I hi, K key, At at)
{
    while (lo < hi) {
        const I mid = (lo + hi + 1) >> 1;
        if (at(mid) <= key) lo = mid; else hi = mid - 1;
    }
    return lo;
}

/* The lane of output tile t (kTile bytes a tile), for `count` units of which unit i begins at output byte starts[i] and
 * `total` output bytes: tile_first[t] = the last unit that begins at or before the tile's first byte; for the entry behind the
 * last used tile the last unit; nothing for a t further behind, or without units.  It stores the entry itself: a caller that
 * stored a returned value loaded its table pointers from the kernel's arguments only behind the branches, two dependent loads
 * more than the tile kernels had.  A template on the tile size so that the division stays a shift. */
template <uint32_t kTile>
__device__ __forceinline__ void tile_first_of(const unsigned long long* starts, uint64_t count, uint64_t total, uint64_t t,
                                              unsigned long long* tile_first)
{
    const uint64_t used = (total + kTile - 1) / kTile;
    if (t > used || count == 0) return;
    if (t == used) { tile_first[t] = count - 1; return; }
    tile_first[t] = last_le((uint64_t)0, count - 1, t * kTile, [&](uint64_t i) { return (uint64_t)starts[i]; });
}

constexpr int kBatch = 4;                         /* chunks whose loads a copy lane issues together */
constexpr int kSlowBatch = 4;                     /* listed slow chunks a group of sixteen lanes takes together */

/* The batches of a workgroup of kLanes lanes over the `tlen` output bytes at `out` (16-byte aligned), kChunks chunks a lane:
 * lane t takes the chunks at r = 16 (t + kLanes k), k in [0, kChunks).  locate(r, tag, s) -> bool is asked for every chunk
 * that begins inside the range, in rising k: whether out[r, r + 16) is src[s, s + 16) and all of it lies inside the range; it
 * leaves in `tag` what the kernel wants to know of a chunk that is not.  defer(r, tag) gets each of those, behind the
 * stores of its batch.  The loads stay in the first half of a batch and the stores in the second: that is what keeps kB
 * chunks' loads in flight. */
template <int kLanes, int kChunks, int kB = kBatch, class Locate, class Defer>
__device__ __forceinline__ void copy_batches(const uint8_t* src, uint8_t* out, uint32_t tlen, Locate locate, Defer defer)
{
    static_assert(kChunks % kB == 0, "whole batches");
#pragma unroll 1
    for (int b = 0; b < kChunks; b += kB) {
        u32x4 va[kB], vb[kB];
        uint32_t sh[kB], tag[kB];
        bool simple[kB], in[kB];
#pragma unroll
        for (int u = 0; u < kB; ++u) {
            const uint32_t r = 16u * (threadIdx.x + (uint32_t)kLanes * (uint32_t)(b + u));
            simple[u] = false; sh[u] = 0; tag[u] = 0;
            va[u] = zero4(); vb[u] = zero4();
            in[u] = r < tlen;
            if (in[u]) {
                uint64_t s = 0;
                if (locate(r, tag[u], s)) {
                    simple[u] = true;
                    load16_pair(src, s, va[u], vb[u], sh[u]);
                }
            }
        }
        /* s_waitcnt vmcnt(0), once for the batch's loads.  Left to the compiler, the wait is placed in front of each chunk's
         * realign where no register copy happens to force it earlier, and there it also waits for the store of the chunk
         * before: the batch's stores would go out one at a time. */
        __builtin_amdgcn_s_waitcnt(0x0F70);
#pragma unroll
        for (int u = 0; u < kB; ++u) {
            const uint32_t r = 16u * (threadIdx.x + (uint32_t)kLanes * (uint32_t)(b + u));
            if (simple[u]) arena_store16(out + r, realign(va[u], vb[u], sh[u]));
            else if (in[u]) defer(r, tag[u]);
        }
    }
}

/* The list of a tile's slow chunks in LDS, an entry a chunk: the chunk's number in the tile | tag << 12, the tag being the
 * number in the tile of the unit the chunk begins in (a unit has a byte or more).  kTile: the tile's bytes. */
template <uint32_t kTile>
__device__ __forceinline__ void slow_push(uint32_t* s_slow, uint32_t& s_nslow, uint32_t r, uint32_t tag)
{
    static_assert(kTile / 16 <= (1u << 12) && kTile <= (1u << 20), "a slow chunk and its tag share a word");
    s_slow[atomicAdd(&s_nslow, 1u)] = (r >> 4) | (tag << 12);
}

/* ... and the workgroup's pass over the `nslow` entries (behind a barrier that follows the last slow_push): kSlow kLanes / 16
 * chunks at a time -- sixty-four with 256 lanes -- a lane a byte of kSlow of them, byte(tag, cur) being output byte cur of a
 * chunk with that tag; the sixteen lanes of a chunk put their bytes together and the first stores them.  The tile is
 * out[t0, t0 + tlen), and its last chunk is stored byte-exactly. */
template <int kLanes, int kSlow = kSlowBatch, class Byte>
__device__ __forceinline__ void copy_slow_list(const uint32_t* s_slow, uint32_t nslow, uint8_t* out, uint64_t t0, uint32_t tlen,
                                               Byte byte)
{
#pragma unroll 1
    for (uint32_t base = 0; base < nslow; base += kSlow * (kLanes / 16)) {
        const uint32_t b = threadIdx.x & 15u;
        uint32_t v[kSlow], r[kSlow], len[kSlow];
#pragma unroll
        for (int u = 0; u < kSlow; ++u) {
            const uint32_t c = base + (uint32_t)u * (kLanes / 16) + (threadIdx.x >> 4);
            v[u] = 0; r[u] = 0; len[u] = 0;
            if (c < nslow) {
                const uint32_t e = s_slow[c];
                r[u] = (e & 0xFFFu) << 4;
                len[u] = tlen - r[u] < 16 ? tlen - r[u] : 16u;
                if (b < len[u]) v[u] = byte(e >> 12, t0 + r[u] + b);
            }
        }
#pragma unroll
        for (int u = 0; u < kSlow; ++u) {
            if (!len[u]) continue;                                    /* (the sixteen lanes of a chunk agree) */
            uint32_t w = v[u] << (8u * (b & 3u));
            w |= __shfl_xor(w, 1, 16);
            w |= __shfl_xor(w, 2, 16);
            u32x4 x;
            x.x = __shfl(w, 0, 16); x.y = __shfl(w, 4, 16); x.z = __shfl(w, 8, 16); x.w = __shfl(w, 12, 16);
            if (len[u] == 16) { if (b == 0) arena_store16(out + t0 + r[u], x); }
            else if (b < len[u]) out[t0 + r[u] + b] = (uint8_t)v[u];  /* the output's end: these bytes and no others */
        }
    }
}

} // namespace hbs
#endif
