/* hbs_lenpref.h -- host-visible launchers of hbs_annexb_to_lenpref / hbs_lenpref_to_annexb (hbs_lenpref.hip). */
#ifndef HBS_LENPREF_H
#define HBS_LENPREF_H

#include <hip/hip_runtime_api.h>
#include "hbs_pieces.h"

namespace hbs {

constexpr int kLenprefNalsPerBlock = 2048;           /* forward plan: 256 lanes x 8 consecutive NALs        */
constexpr int kLenprefSamplesPerBlock = 256;         /* reverse plan: one lane per sample                   */

struct A2lArgs {
    uint64_t n;                                       /* stream bytes                                          */
    const hbs_nal_entry* index; uint64_t n_nals;
    const uint8_t* keep;                              /* NULL: all                                             */
    const uint32_t* nal_au; uint64_t n_aus;           /* nal_au NULL: no sample table                          */
    unsigned long long* sample_off;                   /* nullable                                              */
    uint64_t out_cap;
    hbs_nal_entry* index_out;                         /* nullable                                              */
    hbs_summary* summary;
    PieceTable t;
    unsigned long long* part;       /* 8 per plan block: record bytes, kept NALs, kept rbsp bytes, 1 if anything was wrong */
    hipEvent_t ev_begin, ev_end;    /* when non-null: recorded around the call's kernels               */
};

struct L2aArgs {
    uint64_t n;                                       /* input bytes                                           */
    uint32_t length_size;                             /* bytes of a length field: 1, 2 or 4                    */
    const unsigned long long* sample_off; const unsigned long long* sample_size; uint64_t n_samples;
    uint64_t nal_cap, out_cap;
    uint64_t piece_cap;                               /* records the piece table holds: min(nal_cap, out_cap / start code), 0 plan-only */
    unsigned long long* sample_off_out;               /* nullable                                              */
    hbs_summary* summary;
    PieceTable t;
    unsigned long long* part;       /* 8 per plan block: output bytes, records, -, 1 + the lowest malformed sample (0: none) */
    unsigned long long* samp;       /* 2 per sample: its output bytes, its records                                          */
    hipEvent_t ev_begin, ev_end;
};

/* the scratch the calls need, sized by n_nals / n_samples and nal_cap, and by t.tiles */
inline void lay_a2l(Carver& w, A2lArgs& a)
{
    const uint64_t blocks = (a.n_nals + kLenprefNalsPerBlock - 1) / kLenprefNalsPerBlock;
    a.part = w.take<unsigned long long>(blocks * 64);
    lay_pieces(w, a.t, a.t.out ? a.n_nals : 0);            /* (a plan-only call fills no piece table) */
}

inline void lay_l2a(Carver& w, L2aArgs& a)
{
    const uint64_t blocks = (a.n_samples + kLenprefSamplesPerBlock - 1) / kLenprefSamplesPerBlock;
    a.part = w.take<unsigned long long>(blocks * 64);
    a.samp = w.take<unsigned long long>(a.n_samples * 16);
    lay_pieces(w, a.t, a.piece_cap);
}

hipError_t launch_annexb_to_lenpref(const A2lArgs& a, hipStream_t st);
hipError_t launch_lenpref_to_annexb(const L2aArgs& a, hipStream_t st);

} // namespace hbs
#endif
