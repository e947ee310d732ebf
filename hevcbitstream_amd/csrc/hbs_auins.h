/*
 * hbs_auins.h -- hbs_au_insert (include/hevcbitstream_amd.h): the access-unit delimiter rule as ONE host/device inline
 * function -- auins_aud_word gives the seven bytes of an inserted AUD; the kernels of hbs_auins.hip, hbs_aud_nal_host and the
 * tests all run it -- and the host-visible launcher.  Everything above the launcher compiles with plain g++.
 */
#ifndef HBS_AUINS_H
#define HBS_AUINS_H

#include "hbs_common.h"
#ifdef __HIPCC__
#include "hbs_pieces.h"
#endif

namespace hbs {

constexpr int kAuinsNalsPerBlock = 2048;            /* NAL side: 256 lanes x 8 consecutive NALs                      */
constexpr int kAuinsAusPerBlock = 256;              /* AU side: one AU a lane                                        */
constexpr uint32_t kAuinsAudBytes = 7;
constexpr uint32_t kAuinsFlags = HBS_AUINS_AUD | HBS_AUINS_PARAM_SETS | HBS_AUINS_PARAM_SETS_FIRST;

/* primary_pic_type of the AUD in front of an AU whose independent slices have the types in slice_types (bit t: type t) */
HBS_HD uint32_t auins_pic_type(uint32_t slice_types)
{
    if (slice_types == 4u) return 0u;                                       /* I only  */
    if (slice_types != 0u && (slice_types & 1u) == 0u) return 1u;           /* P and I */
    return 2u;
}

/* the inserted AUD 00 00 00 01 46 T X, byte i in bits [8 i, 8 i + 8) */
HBS_HD uint64_t auins_aud_word(int32_t temporal_id_plus1, uint32_t slice_types)
{
    const uint64_t T = (uint32_t)temporal_id_plus1 & 7u, X = (auins_pic_type(slice_types) << 5) | 0x10u;
    return 0x0000004601000000ull | (T << 40) | (X << 48);
}

inline int auins_aud_host(int temporal_id_plus1, uint32_t slice_types, uint8_t out[7])
{
    if (!out) return HBS_E_ARG;
    const uint64_t w = auins_aud_word(temporal_id_plus1, slice_types);
    for (int i = 0; i < 7; ++i) out[i] = (uint8_t)(w >> (8 * i));
    return 0;
}

#ifdef __HIPCC__
/* what the count kernel decided for an AU of the range, once */
struct alignas(16) AuinsDec {
    uint32_t q[3];                  /* number + 1 of the VPS / SPS / PPS NAL a copy of which is inserted (0: none)   */
    uint32_t bits;                  /* 1: an AUD is inserted, 2: the AU begins with an AUD of its own                */
    unsigned long long ins_bytes;   /* bytes the AU's insertions take                                                */
    unsigned long long ins_rbsp;    /* ... and the sum of their rbsp_len                                             */
};
/* where the place kernel put the AU */
struct alignas(16) AuinsPl {
    unsigned long long ex_bytes;    /* bytes inserted in front of the AU                                             */
    unsigned long long ex_rbsp;     /* rbsp_len of the NALs inserted in front of the AU                              */
    uint32_t ex_nals;               /* NALs inserted in front of the AU                                              */
    uint32_t first_nal;
    uint32_t pad[2];
};

struct AuinsArgs {
    uint64_t n;                                       /* stream bytes (the stream is t.src)                          */
    const hbs_nal_entry* index; const hbs_parsed_nal* parsed; uint64_t n_nals;
    const hbs_access_unit* au; const uint32_t* nal_au; uint64_t n_aus;
    uint64_t a0, cnt;                                 /* the clipped range                                           */
    uint32_t flags;
    uint64_t out_cap, index_cap;
    hbs_nal_entry* index_out; uint32_t* nal_src; uint32_t* nal_au_out; hbs_access_unit* au_out;    /* nullable       */
    hbs_summary* summary;
    PieceTable t;                   /* pieces: the range's bytes in front of the first insertion, then per AU with insertions
                                       its AUD, its sets and the verbatim bytes up to the next such AU; t.tiles covers out_cap */
    /* scratch (lay_auins) */
    unsigned long long* part_n;     /* 8 per NAL block: rbsp_len of the range's NALs, inconsistent                   */
    uint32_t* last_n;               /* 4 per NAL block: the last VPS / SPS / PPS (number + 1) of the block, then in front of it */
    uint32_t* au_q;                 /* 4 per AU: the last VPS / SPS / PPS in front of the AU's picture NAL inside that NAL's block */
    unsigned long long* part_a;     /* 8 per AU block: inserted bytes, AUDs, sets, AUs with insertions, inserted rbsp_len, inconsistent */
    AuinsDec* dec;                  /* n_aus                                                                         */
    AuinsPl* pl;                    /* n_aus (a plan-only call places nothing)                                       */
    unsigned long long* ctl2;       /* 8: first NAL of the range, one past its last, unit_begin of its first AU, M, range rbsp_len */
    hipEvent_t ev_begin, ev_end;
};

inline uint64_t auins_nal_blocks(uint64_t n_nals) { return n_nals / kAuinsNalsPerBlock + 1; }      /* positions 0 .. n_nals */
inline uint64_t auins_au_blocks(uint64_t n_aus) { return (n_aus + kAuinsAusPerBlock - 1) / kAuinsAusPerBlock; }

/* the scratch the call needs, sized by a.n_nals, a.n_aus, a.cnt and a.t.tiles */
inline void lay_auins(Carver& w, AuinsArgs& a)
{
    a.part_n = w.take<unsigned long long>(auins_nal_blocks(a.n_nals) * 64);
    a.last_n = w.take<uint32_t>(auins_nal_blocks(a.n_nals) * 16);
    a.au_q = w.take<uint32_t>(a.n_aus * 16);
    a.part_a = w.take<unsigned long long>(auins_au_blocks(a.n_aus) * 64);
    a.dec = w.take<AuinsDec>(a.n_aus * sizeof(AuinsDec));
    a.pl = w.take<AuinsPl>((a.t.out ? a.n_aus : 0) * sizeof(AuinsPl));
    a.ctl2 = w.take<unsigned long long>(64);
    const uint64_t piece_cap = a.t.out ? 5 * a.cnt + 1 : 0;         /* an AUD, three sets and a verbatim run an AU */
    lay_pieces(w, a.t, piece_cap);
    a.t.piece_lit = w.take<unsigned long long>((piece_cap + 1) * 8);
}
hipError_t launch_au_insert(const AuinsArgs& a, hipStream_t st);
#endif

} // namespace hbs
#endif
