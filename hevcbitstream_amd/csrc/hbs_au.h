/*
 * hbs_au.h -- hbs_access_units / hbs_au_keep (include/hevcbitstream_amd.h): the per-NAL classification, the picture
 * rules and the scan operators, as host/device inline functions (they compile with g++ for single-stepping), and the
 * host-visible launchers of hbs_au.hip.
 *
 * Every "the last such NAL in front of k" of the specification is an exclusive max-scan of `number + 1` (0 = none);
 * the AU number is a sum-scan of the AU starts; the anchors' PicOrderCntMsb is a segmented sum (au_seg_combine).
 */
#ifndef HBS_AU_H
#define HBS_AU_H

#include "hbs_common.h"

namespace hbs {

constexpr int kAuNalsPerBlock = 2048;               /* 256 lanes x 8 steps, one NAL per lane and step */

/* ---- the 16-byte digest of a NAL: all that the passes behind the first one look at ---- */
struct AuDigest {
    uint32_t cls;                                    /* AU_C_* */
    int32_t lsb;                                     /* slice_pic_order_cnt_lsb as the parse reports it */
    uint64_t end;                                    /* index[k].end */
};

constexpr uint32_t AU_C_TYPE1 = 0x7Fu;               /* nal_unit_type + 1 (0: type -1)                        */
constexpr uint32_t AU_C_LAYER0 = 1u << 7;            /* nuh_layer_id == 0                                     */
constexpr int      AU_C_TID_SHIFT = 8;               /* 3 bits: nuh_temporal_id_plus1                         */
constexpr uint32_t AU_C_FIRST = 1u << 11;            /* first_slice_segment_in_pic_flag != 0                  */
constexpr uint32_t AU_C_INDEP = 1u << 12;            /* dependent_slice_segment_flag == 0                     */
constexpr int      AU_C_STYPE_SHIFT = 13;            /* 2 bits: slice_type 0..2, 3: anything else             */
constexpr uint32_t AU_C_DAMAGED = 1u << 15;
constexpr uint32_t AU_C_SPS_SLOT = 1u << 16;         /* type 33 with struct_off != ~0                         */
constexpr int      AU_C_LOG2_SHIFT = 17;             /* 4 bits: clamp(log2_max_pic_order_cnt_lsb_minus4, 0, 12) of that SPS */

HBS_HD uint32_t au_classify(int32_t rc, int32_t type, int32_t layer, int32_t tid1, int has_slot, int32_t sps_log2m4,
                            int32_t first_flag, int32_t dependent_flag, int32_t slice_type)
{
    const int32_t t = (type < 0 || type > 63) ? -1 : type;
    uint32_t c = (uint32_t)(t + 1);
    if (layer == 0) c |= AU_C_LAYER0;
    c |= ((uint32_t)tid1 & 7u) << AU_C_TID_SHIFT;
    if (first_flag != 0) c |= AU_C_FIRST;
    if (dependent_flag == 0) c |= AU_C_INDEP;
    c |= ((slice_type >= 0 && slice_type <= 2) ? (uint32_t)slice_type : 3u) << AU_C_STYPE_SHIFT;
    if (t < 0 || (rc < 0 && t < 35)) c |= AU_C_DAMAGED;
    if (t == 33 && has_slot) {
        const int32_t v = sps_log2m4 < 0 ? 0 : (sps_log2m4 > 12 ? 12 : sps_log2m4);
        c |= AU_C_SPS_SLOT | ((uint32_t)v << AU_C_LOG2_SHIFT);
    }
    return c;
}

HBS_HD int au_type(uint32_t c) { return (int)(c & AU_C_TYPE1) - 1; }
HBS_HD int au_tid1(uint32_t c) { return (int)((c >> AU_C_TID_SHIFT) & 7u); }
HBS_HD bool au_is_vcl(uint32_t c) { return (c & AU_C_LAYER0) && au_type(c) >= 0 && au_type(c) <= 31; }
HBS_HD bool au_is_first(uint32_t c) { return au_is_vcl(c) && (c & AU_C_FIRST); }
/* 7.4.2.4.4: the NALs that may begin an access unit */
HBS_HD bool au_is_cand(uint32_t c)
{
    if (au_is_first(c)) return true;
    if (!(c & AU_C_LAYER0)) return false;
    const int t = au_type(c);
    return (t >= 32 && t <= 35) || t == 39 || (t >= 41 && t <= 44) || (t >= 48 && t <= 55);
}
HBS_HD bool au_is_eos(uint32_t c) { return au_type(c) == 36; }

/* v1 / c1: number + 1 of the last VCL / CAND NAL in front of NAL k (0: none) */
HBS_HD bool au_starts(uint32_t c, uint64_t k, uint32_t v1, uint32_t c1) { return k == 0 || (au_is_cand(c) && c1 <= v1); }
/* the picture NAL = the first VCL NAL of its AU: a first slice segment always is; any other VCL NAL is when a CAND NAL
 * (which began the AU) lies behind the last VCL NAL, or when no VCL NAL lies in front at all (the AU that NAL 0 began) */
HBS_HD bool au_is_picture(uint32_t c, uint32_t v1, uint32_t c1) { return au_is_vcl(c) && ((c & AU_C_FIRST) || c1 > v1 || v1 == 0); }

/* HBS_AU_IRAP / IDR / ANCHOR of a picture NAL */
HBS_HD uint32_t au_picture_flags(uint32_t c)
{
    const int t = au_type(c);
    uint32_t f = 0;
    if (t >= 16 && t <= 23) f |= HBS_AU_IRAP;
    if (t == 19 || t == 20) f |= HBS_AU_IDR;
    if (au_tid1(c) == 1 && !(t >= 6 && t <= 9) && !(t <= 14 && (t & 1) == 0)) f |= HBS_AU_ANCHOR;
    return f;
}
/* NoRaslOutputFlag = 1.  pic_seen: a picture lies in front (or the carry says so); eos_pending: an end-of-sequence NAL
 * lies behind the last picture in front (or, without one in this call, anywhere in front, or the carry says so) */
HBS_HD bool au_cvs_start(uint32_t c, bool pic_seen, bool eos_pending)
{
    const int t = au_type(c);
    if (t >= 16 && t <= 20) return true;
    if (t >= 21 && t <= 23) return !pic_seen || eos_pending;
    return false;
}
/* 8.3.1: what the picture adds to its anchor's PicOrderCntMsb */
HBS_HD int32_t au_poc_delta(int32_t prev_lsb, int32_t lsb, uint32_t log2m4)
{
    const int64_t mx = (int64_t)1 << (4 + log2m4), p = prev_lsb, l = lsb;
    if (l < p && p - l >= mx / 2) return (int32_t)mx;
    if (l > p && l - p > mx / 2) return -(int32_t)mx;
    return 0;
}

/* segmented sum: (reset, sum) o (reset, sum); a reset element's sum is the value behind it */
struct AuSeg { uint32_t reset; uint32_t sum; };
HBS_HD AuSeg au_seg_combine(AuSeg a, AuSeg b)
{
    AuSeg r;
    r.reset = a.reset | b.reset;
    r.sum = b.reset ? b.sum : a.sum + b.sum;
    return r;
}

#ifdef __HIPCC__
struct AuArgs {
    const hbs_nal_entry* index; const hbs_parsed_nal* parsed; const hbs_slice_compact* compact; const uint8_t* structs;
    uint64_t n_nals, sps_off;
    hbs_au_carry initial;
    hbs_access_unit* au; uint64_t au_cap; uint32_t* nal_au; hbs_au_carry* carry_out; hbs_summary* summary;
    /* scratch (lay_access_units) */
    AuDigest* digest;               /* n_nals                                                                   */
    uint32_t* part1;                /* 8 per block: last VCL, CAND, EOS, SPS with a slot (number + 1), VCL NALs  */
    uint32_t* part2;                /* 8 per block: AU starts, pictures, last start, last picture, last anchor   */
    uint32_t* part3;                /* 8 per block: CVS starts, the anchors' msb as (reset, sum)                 */
    uint32_t* lead;                 /* 8 per block: what the block adds to the AU that an earlier block began    */
    uint32_t* ctl;                  /* 64: error, totals                                                         */
    hipEvent_t ev_begin, ev_end;
};
/* the scratch the call needs, sized by a.n_nals */
inline void lay_access_units(Carver& w, AuArgs& a)
{
    const uint64_t blocks = (a.n_nals + kAuNalsPerBlock - 1) / kAuNalsPerBlock;
    a.digest = w.take<AuDigest>(a.n_nals * sizeof(AuDigest));
    a.part1 = w.take<uint32_t>(blocks * 32);
    a.part2 = w.take<uint32_t>(blocks * 32);
    a.part3 = w.take<uint32_t>(blocks * 32);
    a.lead = w.take<uint32_t>(blocks * 32);
    a.ctl = w.take<uint32_t>(256);
}
hipError_t launch_access_units(const AuArgs& a, hipStream_t st);

struct AuKeepArgs {
    const uint32_t* nal_au; const hbs_parsed_nal* parsed; uint64_t n_nals, first_au, au_count; int flags;
    uint8_t* keep;
    uint32_t* sets;                 /* 4: number + 1 of the last VPS, SPS, PPS in front of the range (scratch, zeroed by the call) */
};
hipError_t launch_au_keep(const AuKeepArgs& a, hipStream_t st);
#endif

} // namespace hbs
#endif
