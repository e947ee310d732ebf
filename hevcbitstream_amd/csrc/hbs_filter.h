/* hbs_filter.h -- host-visible launcher of hbs_filter_annexb (hbs_filter.hip). */
#ifndef HBS_FILTER_H
#define HBS_FILTER_H

#include <hip/hip_runtime_api.h>
#include "hbs_pieces.h"

namespace hbs {

constexpr int kFilterNalsPerBlock = 2048;            /* plan: 256 lanes x 8 consecutive NALs         */

struct FilterArgs {
    uint64_t n;                                       /* stream bytes (the stream is t.src)           */
    const hbs_nal_entry* index; uint64_t n_nals;
    hbs_nal_filter rule; int use_rule;                /* use_rule 0: keep = d_keep[k] != 0            */
    const uint8_t* keep;
    uint64_t out_cap;
    hbs_nal_entry* index_out;                         /* nullable                                     */
    hbs_summary* summary;
    PieceTable t;                   /* a piece per kept non-empty unit, prefix 0; t.ctl[3]: kept NALs; t.tiles covers min(n, out_cap) */
    unsigned long long* part;       /* 8 per plan block: unit bytes, kept NALs, kept rbsp bytes, kept non-empty units, inconsistent */
    hipEvent_t ev_begin, ev_end;    /* when non-null: recorded around the call's kernels                              */
};

/* the scratch the call needs, sized by a.n_nals and a.t.tiles */
inline void lay_filter(Carver& w, FilterArgs& a)
{
    const uint64_t blocks = (a.n_nals + kFilterNalsPerBlock - 1) / kFilterNalsPerBlock;
    a.part = w.take<unsigned long long>(blocks * 64);       /* 8 words a plan block: 4 sums, the "inconsistent" flag, 3 spare */
    lay_pieces(w, a.t, a.n_nals);
}

hipError_t launch_filter_annexb(const FilterArgs& a, hipStream_t st);

} // namespace hbs
#endif
