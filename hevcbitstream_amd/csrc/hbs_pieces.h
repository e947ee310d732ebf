/* hbs_pieces.h -- the table of "pieces" a plan ends in and the copy over it (hbs_pieces.hip): what hbs_filter_annexb,
 * hbs_annexb_to_lenpref, hbs_lenpref_to_annexb and hbs_au_insert share. */
#ifndef HBS_PIECES_H
#define HBS_PIECES_H

#include <hip/hip_runtime_api.h>
#include "hbs_common.h"

namespace hbs {

constexpr uint64_t kPieceTileBytes = 64 * 1024;      /* copy: output bytes of one workgroup */

/* What the copy kernel works on.  Piece j is the output bytes [piece_out[j], piece_out[j + 1]): `prefix` literal bytes, then
 * source bytes; output byte o of its payload is src[o + piece_delta[j]].  The copy reads ctl[0..2]; the other five control
 * words are the caller's (the filter keeps its kept NALs in ctl[3]). */
struct PieceTable {
    const uint8_t* src;
    uint8_t* out;                   /* NULL: plan only                                                              */
    uint32_t prefix;                /* bytes of the literal in front of each payload: length_size / startcode_bytes;
                                       0: none (a unit of the filter)                                               */
    int prefix_is_length;           /* 1: the payload's length, big-endian; 0: 00 .. 00 01                          */
    unsigned long long* piece_lit;  /* NULL, or pieces words (prefix 0 then): piece j begins with its own literal of
                                       piece_lit[j] >> 56 bytes (at most 7), byte i of it in bits [8 i, 8 i + 8); a piece of
                                       such a table may be empty (hbs_au_insert: an AUD, a start code, nothing)              */
    unsigned long long* ctl;        /* 8: error, output bytes, pieces                                               */
    unsigned long long* piece_out;  /* pieces + 1: output offset of piece j (then the total)                        */
    unsigned long long* piece_delta;/* pieces: source offset minus output offset of its payload                     */
    unsigned long long* tile_first; /* tiles + 1: the piece the output tile's first byte lies in                    */
    uint64_t tiles;                 /* output tiles the grid covers                                                 */
};

inline void lay_pieces(Carver& w, PieceTable& t, uint64_t piece_cap)
{
    t.ctl = w.take<unsigned long long>(64);
    t.piece_out = w.take<unsigned long long>((piece_cap + 1) * 8);
    t.piece_delta = w.take<unsigned long long>(piece_cap * 8);
    t.tile_first = w.take<unsigned long long>((t.tiles + 1) * 8);
}

/* the output tiles a grid covers for an output of at most `reach` bytes (what a grid can hold is far beyond device memory) */
inline uint64_t piece_tiles(uint64_t reach)
{
    const uint64_t t = reach / kPieceTileBytes + (reach % kPieceTileBytes ? 1 : 0);
    return t < 0x7FFFFFFFull ? t : 0x7FFFFFFFull;
}

/* behind the plan, on its stream: the tile kernel and the copy kernel (nothing when t.tiles is 0) */
hipError_t copy_pieces(const PieceTable& t, hipStream_t st);

} // namespace hbs
#endif
