/* hbs_filter.h -- host-visible launcher of hbs_filter_annexb (hbs_filter.hip). */
#ifndef HBS_FILTER_H
#define HBS_FILTER_H

#include <hip/hip_runtime_api.h>
#include "hbs_common.h"

namespace hbs {

constexpr int kFilterNalsPerBlock = 2048;            /* plan: 256 lanes x 8 consecutive NALs         */
constexpr uint64_t kFilterTileBytes = 64 * 1024;     /* copy: output bytes of one workgroup          */

struct FilterArgs {
    const uint8_t* stream; uint64_t n;
    const hbs_nal_entry* index; uint64_t n_nals;
    hbs_nal_filter rule; int use_rule;                /* use_rule 0: keep = d_keep[k] != 0            */
    const uint8_t* keep;
    uint8_t* out; uint64_t out_cap;                   /* out NULL: plan only                          */
    hbs_nal_entry* index_out;                         /* nullable                                     */
    hbs_summary* summary;
    /* scratch (lay_filter) */
    unsigned long long* part;       /* 8 per plan block: unit bytes, kept NALs, kept rbsp bytes, kept non-empty units, inconsistent */
    unsigned long long* ctl;        /* 8: error, output bytes, non-empty kept units, kept NALs                        */
    unsigned long long* kept_out;   /* n_nals + 1: output offset of the j-th non-empty kept unit (then the total)     */
    unsigned long long* kept_delta; /* n_nals: its stream offset minus its output offset                              */
    unsigned long long* tile_first; /* tiles + 1: the unit the output tile's first byte lies in                       */
    uint64_t tiles;                 /* output tiles the grid covers: ceil(min(n, out_cap) / kFilterTileBytes)         */
    hipEvent_t ev_begin, ev_end;    /* when non-null: recorded around the call's kernels                              */
};

/* the scratch the call needs, sized by a.n_nals and a.tiles */
inline void lay_filter(Carver& w, FilterArgs& a)
{
    const uint64_t blocks = (a.n_nals + kFilterNalsPerBlock - 1) / kFilterNalsPerBlock;
    a.part = w.take<unsigned long long>(blocks * 64);       /* 8 words a plan block: 4 sums, the "inconsistent" flag, 3 spare */
    a.ctl = w.take<unsigned long long>(64);
    a.kept_out = w.take<unsigned long long>((a.n_nals + 1) * 8);
    a.kept_delta = w.take<unsigned long long>(a.n_nals * 8);
    a.tile_first = w.take<unsigned long long>((a.tiles + 1) * 8);
}

hipError_t launch_filter_annexb(const FilterArgs& a, hipStream_t st);

} // namespace hbs
#endif
