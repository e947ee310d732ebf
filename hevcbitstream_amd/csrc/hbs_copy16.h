/*
 * hbs_copy16.h -- device-only, for .hip files: what the copies that take one lane per aligned 16-byte output chunk share
 * (hbs_pieces.hip, hbs_rtp.hip, hbs_tsmux.hip, hbs_ts.hip, hbs_mp4.hip, hbs_mp4prot.hip).  The fast path of a chunk that lies inside one run of source bytes:
 * load16_pair, realign, arena_store16 (hbs_wave.h).  The slow path of a chunk that holds other bytes or spans runs: pack_byte
 * for each byte, then store_chunk.  last_le finds the unit a chunk lies in, tile_first_of the unit an output tile begins in.
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

} // namespace hbs
#endif
