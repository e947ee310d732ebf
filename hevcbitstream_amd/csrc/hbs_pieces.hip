/*
 * hbs_pieces.hip -- copy_pieces: the copy over a table of "pieces" (hbs_pieces.h) -- a short literal prefix, possibly of no
 * bytes, followed by a run of source bytes at its own byte misalignment.  One copy for hbs_filter_annexb (hbs_filter.hip: a
 * kept unit is a piece without a prefix), hbs_annexb_to_lenpref and hbs_lenpref_to_annexb (hbs_lenpref.hip) and hbs_au_insert
 * (hbs_auins.hip: every piece with a literal of its own, of 0 to 7 bytes); their plans fill the table.  Two launches, neither
 * of which waits for another workgroup:
 *
 *   k_piece_tiles    one lane per 64 KiB output tile: binary search of the piece its first byte lies in
 *   k_piece_copy     one workgroup per output tile: each lane takes 16-byte output chunks 4 KiB apart and finds the piece of
 *                    each (the tile's pieces are staged in LDS; more than 2 048 are read from memory), in the skeleton that
 *                    hbs_copy16.h describes, its batch loop written out here: the fast path for the chunks inside one
 *                    payload; a chunk that holds a prefix byte or spans pieces, and the output's last chunk, is marked in a
 *                    bit mask and assembled byte by byte behind them by the lane that met it (copy_chunk_bytes), stored
 *                    byte-exact.  A payload of any size spreads over the
 *                    tiles it covers.  <kMode>: kPieceBare for a table without prefixes, where all that is about them folds
 *                    away; kPiecePrefix for one prefix form a table; kPieceLiteral for a literal a piece (piece_lit), whose
 *                    length is staged next to the piece and whose bytes are read where a chunk holds some.
 *
 * The chunk's loads, realignment and searches are hbs_copy16.h, which the other copies share.
 *
 * Traffic: the payloads read once and written once, 16 B a piece and 8 B a tile of scratch read.
 */
#include <hip/hip_runtime.h>
#include "hbs_pieces.h"
#include "hbs_copy16.h"

namespace hbs {
namespace {

constexpr int kCT = 256;                                              /* lanes of the copy workgroup             */
constexpr uint32_t kTile = (uint32_t)kPieceTileBytes;
constexpr int kChunks = (int)(kPieceTileBytes / 16 / kCT);            /* 16-byte output chunks a copy lane takes */
constexpr uint32_t kLdsPieces = 2048;                                 /* pieces a tile stages in LDS; more: read from memory */
constexpr int32_t kFar = -8;                                          /* a piece that begins this far in front of the tile or
                                                                         further: its prefix (<= 7 bytes) is not in the tile */
enum : int { kPieceBare = 0, kPiecePrefix = 1, kPieceLiteral = 2 };

__global__ __launch_bounds__(256) void k_piece_tiles(PieceTable a)
{
    if (a.ctl[0] != 0) return;
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    tile_first_of<kTile>(a.piece_out, a.ctl[2], a.ctl[1], t, a.tile_first);
}

/* the tile's pieces [j0, j0 + cnt): rel(i) = where piece j0 + i begins, relative to the tile, clamped to [kFar, kTile] (without
 * prefixes to [0, kTile]: where a piece begins in front of the tile says nothing then) */
template <int kMode>
struct TilePieces {
    static constexpr bool kPrefix = kMode != kPieceBare;
    const int32_t* s_bound; const unsigned long long* s_delta;     /* staged: LDS */
    const uint8_t* s_lit;                                          /* kPieceLiteral: the literals' lengths */
    const unsigned long long* piece_out; const unsigned long long* piece_delta; const unsigned long long* piece_lit;
    uint64_t j0, t0;
    bool lds;
    __device__ __forceinline__ int32_t rel(uint32_t i) const
    {
        if (lds) return s_bound[i];
        const uint64_t b = piece_out[j0 + i];
        if (b >= t0) return b - t0 >= kTile ? (int32_t)kTile : (int32_t)(b - t0);
        if (!kPrefix) return 0;
        return t0 - b >= (uint64_t)(-kFar) ? kFar : -(int32_t)(t0 - b);
    }
    __device__ __forceinline__ uint64_t delta(uint32_t i) const { return lds ? s_delta[i] : piece_delta[j0 + i]; }
    __device__ __forceinline__ int32_t lit_bytes(uint32_t i) const { return lds ? (int32_t)s_lit[i] : (int32_t)(piece_lit[j0 + i] >> 56); }
    /* the last piece i in [lo, hi] with rel(i) <= r (rel(lo) <= r holds) */
    __device__ __forceinline__ uint32_t find(uint32_t lo, uint32_t hi, uint32_t r) const
    {
        return last_le(lo, hi, (int32_t)r, [&](uint32_t i) { return rel(i); });
    }
};

/* an output chunk [r, r + len) of the tile that holds prefix bytes or spans pieces (or ends the output): assembled byte by
 * byte, each payload byte loaded from the piece it belongs to, each prefix byte computed */
template <int kMode>
__device__ __forceinline__ void copy_chunk_bytes(const PieceTable& a, const TilePieces<kMode>& tp, uint32_t ip, uint32_t r, uint32_t len)
{
    constexpr bool kPrefix = kMode != kPieceBare;
    uint64_t clo = 0, chi = 0;
    int32_t b0 = tp.rel(ip), b1 = tp.rel(ip + 1);
    uint64_t delta = tp.delta(ip);
    uint64_t plen = 0;
    bool have_len = false;
    int32_t P = kMode == kPiecePrefix ? (int32_t)a.prefix : 0;
    uint64_t lit = 0;
    if (kMode == kPieceLiteral) { lit = a.piece_lit[tp.j0 + ip]; P = (int32_t)(lit >> 56); }
#pragma unroll 1
    for (uint32_t q = 0; q < len; ++q) {
        const int32_t ro = (int32_t)(r + q);
        if (kMode == kPieceLiteral) {          /* (pieces of such a table may be empty) */
            if (ro >= b1) {
                do { ip += 1; b0 = b1; b1 = tp.rel(ip + 1); } while (ro >= b1);
                delta = tp.delta(ip); lit = a.piece_lit[tp.j0 + ip]; P = (int32_t)(lit >> 56);
            }
        } else if (ro >= b1) { ip += 1; b0 = b1; b1 = tp.rel(ip + 1); delta = tp.delta(ip); have_len = false; }
        const int32_t pos = ro - b0;           /* (a piece clamped to kFar: pos >= 8, payload) */
        uint64_t v;
        if (!kPrefix || pos >= P) {
            v = a.src[delta + tp.t0 + (uint32_t)ro];
        } else if (kMode == kPieceLiteral) {
            v = (lit >> (8 * pos)) & 0xFFu;
        } else if (a.prefix_is_length) {
            if (!have_len) { plen = a.piece_out[tp.j0 + ip + 1] - a.piece_out[tp.j0 + ip] - (uint64_t)P; have_len = true; }
            v = (plen >> (8 * (P - 1 - pos))) & 0xFFu;
        } else {
            v = pos == P - 1 ? 1u : 0u;
        }
        if (q < 8) clo |= v << (8 * q); else chi |= v << (8 * (q - 8));
    }
    /* pack_byte and store_chunk (hbs_copy16.h), written out: with the two calls this path compiles to other code, and the
     * filter and length-prefix calls then ran 0.4 to 0.9 % longer (profiles/r16/shared_time.txt) */
    uint8_t* dst = a.out + tp.t0 + r;
    if (len == 16) {
        u32x4 c;
        c.x = (uint32_t)clo; c.y = (uint32_t)(clo >> 32); c.z = (uint32_t)chi; c.w = (uint32_t)(chi >> 32);
        arena_store16(dst, c);
    } else {
        store_pieces(dst, clo, chi, len);
    }
}

template <int kMode>
__global__ __launch_bounds__(kCT) void k_piece_copy(PieceTable a)
{
    constexpr bool kPrefix = kMode != kPieceBare;
    __shared__ int32_t s_bound[kLdsPieces + 1];
    __shared__ unsigned long long s_delta[kLdsPieces];
    __shared__ uint8_t s_lit[kMode == kPieceLiteral ? kLdsPieces : 1];
    if (a.ctl[0] != 0) return;
    const uint64_t total = a.ctl[1];
    const uint64_t t0 = (uint64_t)blockIdx.x * kTile;
    if (t0 >= total) return;
    const uint32_t tlen = total - t0 < kTile ? (uint32_t)(total - t0) : kTile;
    const uint64_t j0 = a.tile_first[blockIdx.x], j1 = a.tile_first[blockIdx.x + 1];
    const uint32_t cnt = (uint32_t)(j1 - j0 + 1);     /* pieces [j0, j1]; piece_out[j1 + 1] exists (the total at the end) */
    TilePieces<kMode> tp;
    tp.s_bound = s_bound; tp.s_delta = s_delta; tp.s_lit = s_lit;
    tp.piece_out = a.piece_out; tp.piece_delta = a.piece_delta; tp.piece_lit = a.piece_lit;
    tp.j0 = j0; tp.t0 = t0; tp.lds = false;
    if (cnt <= kLdsPieces) {
        for (uint32_t i = threadIdx.x; i <= cnt; i += kCT) {
            s_bound[i] = tp.rel(i);
            if (i < cnt) s_delta[i] = a.piece_delta[j0 + i];
            if (kMode == kPieceLiteral && i < cnt) s_lit[i] = (uint8_t)(a.piece_lit[j0 + i] >> 56);
        }
        __syncthreads();
        tp.lds = true;
    }
    const int32_t P = kMode == kPiecePrefix ? (int32_t)a.prefix : 0;
    uint32_t lo = 0;
    uint32_t slow = 0;                        /* chunks done byte by byte, behind the batches: bit b + u */
    uint32_t slow_ip[kChunks];
    /* copy_batches (hbs_copy16.h) written out: with it the filter's row of one ~128-byte NAL in ten ran 1.0 to 1.4 % longer in
     * two samples of two, the other rows of the piece calls shorter by up to 8 % (profiles/r26/copy_time.txt) */
#pragma unroll 1
    for (int b = 0; b < kChunks; b += kBatch) {
        u32x4 va[kBatch], vb[kBatch];
        uint32_t sh[kBatch], ip[kBatch];
        bool simple[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const uint32_t r = 16u * (threadIdx.x + (uint32_t)kCT * (uint32_t)(b + u));
            simple[u] = false; sh[u] = 0; ip[u] = lo;
            va[u] = zero4(); vb[u] = zero4();
            if (r < tlen) {
                lo = tp.find(lo, cnt - 1, r);
                ip[u] = lo;
                if (tlen - r >= 16 && tp.rel(lo + 1) - (int32_t)r >= 16 &&
                    (!kPrefix || (int32_t)r - tp.rel(lo) >= (kMode == kPieceLiteral ? tp.lit_bytes(lo) : P))) {
                    simple[u] = true;
                    load16_pair(a.src, tp.delta(lo) + t0 + r, va[u], vb[u], sh[u]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const uint32_t r = 16u * (threadIdx.x + (uint32_t)kCT * (uint32_t)(b + u));
            if (simple[u]) arena_store16(a.out + t0 + r, realign(va[u], vb[u], sh[u]));
            else if (r < tlen) { slow |= 1u << (b + u); slow_ip[b + u] = ip[u]; }
        }
    }
#pragma unroll 1
    while (slow) {
        const int i = (int)__builtin_ctz(slow);
        slow &= slow - 1;
        const uint32_t r = 16u * (threadIdx.x + (uint32_t)kCT * (uint32_t)i);
        copy_chunk_bytes(a, tp, slow_ip[i], r, tlen - r < 16 ? tlen - r : 16u);
    }
}

} // namespace

hipError_t copy_pieces(const PieceTable& t, hipStream_t st)
{
    if (!t.tiles) return hipSuccess;
    hipLaunchKernelGGL(k_piece_tiles, dim3((unsigned)((t.tiles + 1 + 255) / 256)), dim3(256), 0, st, t);
    if (t.piece_lit) hipLaunchKernelGGL(k_piece_copy<kPieceLiteral>, dim3((unsigned)t.tiles), dim3(kCT), 0, st, t);
    else if (t.prefix) hipLaunchKernelGGL(k_piece_copy<kPiecePrefix>, dim3((unsigned)t.tiles), dim3(kCT), 0, st, t);
    else hipLaunchKernelGGL(k_piece_copy<kPieceBare>, dim3((unsigned)t.tiles), dim3(kCT), 0, st, t);
    return hipSuccess;
}

} // namespace hbs
