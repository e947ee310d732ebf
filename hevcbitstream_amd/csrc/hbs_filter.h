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
    /* scratch (filter_scratch) */
    unsigned long long* part;       /* 8 per plan block: unit bytes, kept NALs, kept rbsp bytes, kept non-empty units, inconsistent */
    unsigned long long* ctl;        /* 8: error, output bytes, non-empty kept units, kept NALs                        */
    unsigned long long* kept_out;   /* n_nals + 1: output offset of the j-th non-empty kept unit (then the total)     */
    unsigned long long* kept_delta; /* n_nals: its stream offset minus its output offset                              */
    unsigned long long* tile_first; /* tiles + 1: the unit the output tile's first byte lies in                       */
    uint64_t tiles;                 /* output tiles the grid covers: ceil(min(n, out_cap) / kFilterTileBytes)         */
    hipEvent_t ev_begin, ev_end;    /* when non-null: recorded around the call's kernels                              */
};

/* scratch the call needs, and where each part lies in it */
struct FilterScratch { uint64_t part, ctl, kept_out, kept_delta, tile_first, total; };
HBS_HD FilterScratch filter_scratch(uint64_t n_nals, uint64_t tiles)
{
    auto r256 = [](uint64_t v) { return (v + 255) & ~255ull; };
    FilterScratch s;
    const uint64_t blocks = (n_nals + kFilterNalsPerBlock - 1) / kFilterNalsPerBlock;
    s.part = 0;
    s.ctl = r256(blocks * 64);                         /* 8 words a plan block: 4 sums, the "inconsistent" flag, 3 spare */
    s.kept_out = s.ctl + 256;
    s.kept_delta = s.kept_out + r256((n_nals + 1) * 8);
    s.tile_first = s.kept_delta + r256(n_nals * 8);
    s.total = s.tile_first + r256((tiles + 1) * 8);
    return s;
}

hipError_t launch_filter_annexb(const FilterArgs& a, hipStream_t st);

} // namespace hbs
#endif
