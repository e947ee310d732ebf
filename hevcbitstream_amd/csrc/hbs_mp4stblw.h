/*
 * hbs_mp4stblw.h -- hbs_mp4_stbl_write (include/hevcbitstream_amd.h): the rules that turn per-sample tables into the six sample
 * table boxes of a progressive MP4 (ISO/IEC 14496-12), as host/device inline functions -- stblw_contiguous and
 * stblw_chunk_start cut the chunks, stblw_place, stblw_dts, stblw_delta and stblw_cts check one sample's offset and times,
 * stblw_run_start begins a run-length entry, stblw_stsz_constant chooses the stsz form, stblw_box_bytes and stblw_layout size
 * and place the boxes and keep every size below 2^32; the kernels of hbs_mp4stblw.hip, the host checks and the tests all run
 * them -- and the host-visible launcher.  Everything above the launcher compiles with plain g++.
 */
#ifndef HBS_MP4STBLW_H
#define HBS_MP4STBLW_H

#include "hbs_mp4.h"

namespace hbs {

constexpr int kSwLanes = 256;                        /* lanes of a workgroup: a sample, a chunk or a run a lane                  */
constexpr uint64_t kSwMax32 = 0xFFFFFFFFull;
constexpr uint32_t kSwNonSync = 0x00010000u;         /* sample_is_non_sync_sample                                                */
/* the boxes in the output's order: the order of the box size error and of stblw_layout */
enum : int { kSwStts = 0, kSwCtts = 1, kSwStss = 2, kSwStsc = 3, kSwStsz = 4, kSwStco = 5, kSwBoxes = 6 };

/* ---- chunks -------------------------------------------------------------------------------------------------------------- */

/* sample k > 0 is contiguous iff it begins where sample k - 1 ends, taken exactly (an end that wraps is no begin) */
HBS_HD bool stblw_contiguous(uint64_t off_prev, uint64_t size_prev, uint64_t off)
{
    return size_prev <= ~off_prev && off == off_prev + size_prev;
}

/* sample k begins a chunk: it is not contiguous (k == s), or it is a multiple of max_chunk_samples behind s = s(k), the last
 * sample at or in front of it that is not contiguous */
HBS_HD bool stblw_chunk_start(uint64_t k, uint64_t s, uint32_t max_chunk_samples)
{
    return k == s || (max_chunk_samples != 0u && (k - s) % max_chunk_samples == 0u);
}

/* ---- one sample ---------------------------------------------------------------------------------------------------------- */

/* o(k) = off + data_offset.  false, a sample error: a size above 2^32 - 1, an o that wraps, o + size at or above 2^62 */
HBS_HD bool stblw_place(uint64_t off, uint64_t size, uint64_t data_offset, uint64_t& o)
{
    o = off + data_offset;
    if (size > kSwMax32 || o < off) return false;
    return o < kMp4TimeLimit && o + size < kMp4TimeLimit;
}

/* a chunk's offset fits its box */
HBS_HD bool stblw_chunk_off_ok(uint64_t o, bool co64) { return co64 || o <= kSwMax32; }

/* dts(k): the table's, or base_time + k * sample_duration (mp4_ruled_dts); false: 2^62 or more */
HBS_HD bool stblw_dts(const uint64_t* dts, uint64_t base_time, uint32_t sample_duration, uint64_t k, uint64_t& t)
{
    if (!dts) return mp4_ruled_dts(base_time, k, sample_duration, t);
    t = dts[k];
    return t < kMp4TimeLimit;
}

/* delta(k) = dts(k + 1) - dts(k); `ruled`: the last sample, or every sample without a d_dts, whose delta is sample_duration.
 * false: outside [0, 2^32 - 1] */
HBS_HD bool stblw_delta(bool ruled, uint64_t t, uint64_t t_next, uint32_t sample_duration, uint64_t& delta)
{
    delta = sample_duration;
    if (ruled) return true;
    if (t_next < t) { delta = 0; return false; }
    delta = t_next - t;
    return delta <= kSwMax32;
}

/* cts(k) = pts - dts(k) (dts below 2^62); false: a pts of 2^62 or more, or a cts outside [-2^31, 2^31 - 1] */
HBS_HD bool stblw_cts(uint64_t pts, uint64_t t, int64_t& cts)
{
    cts = 0;
    if (pts >= kMp4TimeLimit || t >= kMp4TimeLimit) return false;
    cts = (int64_t)pts - (int64_t)t;
    return cts >= -2147483648ll && cts <= 2147483647ll;
}

/* a run-length entry (stts, ctts; the stsc over the chunks' lengths) begins at element i: the first, or a value other than
 * the one in front */
HBS_HD bool stblw_run_start(uint64_t i, uint64_t v, uint64_t v_prev) { return i == 0 || v != v_prev; }

HBS_HD bool stblw_sync(uint32_t flags) { return (flags & kSwNonSync) == 0u; }

/* the tables and the parameters a sample's rules read */
struct StblwIn {
    const uint64_t* off; const uint64_t* size; uint64_t n;
    const uint64_t* dts; const uint64_t* pts; const uint32_t* sflags;     /* nullable */
    uint32_t sample_duration; uint64_t base_time, data_offset;
};

/* dts(k) and delta(k) of sample k < n; false: one of the two breaks its rule */
HBS_HD bool stblw_times(const StblwIn& in, uint64_t k, uint64_t& t, uint64_t& delta)
{
    bool ok = stblw_dts(in.dts, in.base_time, in.sample_duration, k, t);
    const bool ruled = !in.dts || k + 1u == in.n;
    ok &= stblw_delta(ruled, t, ruled ? 0u : in.dts[k + 1u], in.sample_duration, delta);
    return ok;
}

/* everything sample k < n says by itself and against its left neighbour (its chunk needs s(k): stblw_chunk_start) */
struct StblwLane {
    uint64_t z, o, delta; int64_t cts;
    bool bad;                        /* a sample error other than the chunk offset's                                              */
    bool brk;                        /* not contiguous                                                                            */
    bool stts_run, ctts_run;         /* an entry of the box begins here (ctts_run: false without a d_pts)                         */
    bool sync;                       /* listed in the stss (false without d_sample_flags)                                         */
};
HBS_HD void stblw_lane(const StblwIn& in, uint64_t k, StblwLane& l)
{
    const uint64_t off = in.off[k];
    l.z = in.size[k];
    bool ok = stblw_place(off, l.z, in.data_offset, l.o);
    l.brk = k == 0 || !stblw_contiguous(in.off[k - 1u], in.size[k - 1u], off);
    uint64_t t, t_prev = 0, delta_prev = 0;
    ok &= stblw_times(in, k, t, l.delta);
    if (k) (void)stblw_times(in, k - 1u, t_prev, delta_prev);
    l.stts_run = stblw_run_start(k, l.delta, delta_prev);
    l.cts = 0; l.ctts_run = false;
    if (in.pts) {
        int64_t cts_prev = 0;
        ok &= stblw_cts(in.pts[k], t, l.cts);
        if (k) (void)stblw_cts(in.pts[k - 1u], t_prev, cts_prev);
        l.ctts_run = stblw_run_start(k, (uint64_t)l.cts, (uint64_t)cts_prev);
    }
    l.sync = in.sflags && stblw_sync(in.sflags[k]);
    l.bad = !ok;
}

/* ---- the boxes ----------------------------------------------------------------------------------------------------------- */

/* the short stsz: there are samples, none differs from the first in size, and that size is not 0 */
HBS_HD bool stblw_stsz_constant(uint64_t N, uint64_t differ, uint64_t size0) { return N > 0 && differ == 0 && size0 != 0; }

/* the bytes of box b, header included, with `entries` entries (stsz: N); exact in 64 bits for entries below 2^32 */
HBS_HD uint64_t stblw_box_bytes(int b, uint64_t entries, bool constant, bool co64)
{
    switch (b) {
    case kSwStts: case kSwCtts: return 16u + 8u * entries;
    case kSwStss: return 16u + 4u * entries;
    case kSwStsc: return 16u + 12u * entries;
    case kSwStsz: return 20u + (constant ? 0u : 4u * entries);
    default:      return 16u + (co64 ? 8u : 4u) * entries;
    }
}

/* the boxes one behind the other: off[b] the box's first byte, bytes[b] its size (0: not written), total their sum.  Returns
 * 1 + the first box whose size passes 2^32 - 1 (then off, bytes and total mean nothing), 0: none */
HBS_HD uint32_t stblw_layout(const uint64_t entries[kSwBoxes], bool with_ctts, bool with_stss, bool constant, bool co64, uint64_t off[kSwBoxes],
                             uint64_t bytes[kSwBoxes], uint64_t& total)
{
    uint64_t at = 0;
    uint32_t bad = 0;
    for (int b = 0; b < kSwBoxes; ++b) {
        const bool present = b == kSwCtts ? with_ctts : b == kSwStss ? with_stss : true;
        const uint64_t n = present ? stblw_box_bytes(b, entries[b], constant, co64) : 0;
        if (n > kSwMax32 && !bad) bad = 1u + (uint32_t)b;
        off[b] = at; bytes[b] = n;
        at += n;
    }
    total = at;
    return bad;
}

HBS_HD uint32_t stblw_fourcc(int b, bool co64)
{
    switch (b) {
    case kSwStts: return HBS_MP4_FOURCC('s', 't', 't', 's');
    case kSwCtts: return HBS_MP4_FOURCC('c', 't', 't', 's');
    case kSwStss: return HBS_MP4_FOURCC('s', 't', 's', 's');
    case kSwStsc: return HBS_MP4_FOURCC('s', 't', 's', 'c');
    case kSwStsz: return HBS_MP4_FOURCC('s', 't', 's', 'z');
    default:      return co64 ? HBS_MP4_FOURCC('c', 'o', '6', '4') : HBS_MP4_FOURCC('s', 't', 'c', 'o');
    }
}

/* ---- host side ----------------------------------------------------------------------------------------------------------- */

/* hbs_mp4_stbl_write_bytes_host: what no output passes -- an entry a sample in every box; 0 for more samples than a call takes */
inline uint64_t mp4_stbl_write_bytes(uint64_t n_samples, int with_ctts, int with_stss, uint32_t flags)
{
    if (n_samples > kSwMax32) return 0;
    uint64_t total = 0;
    for (int b = 0; b < kSwBoxes; ++b)
        if ((b != kSwCtts || with_ctts) && (b != kSwStss || with_stss)) total += stblw_box_bytes(b, n_samples, false, (flags & HBS_MP4_STBL_CO64) != 0u);
    return total;
}

inline bool mp4_stbl_write_params_ok(const hbs_mp4_stbl_write_params* p)
{
    return p && (p->flags & ~(uint32_t)HBS_MP4_STBL_CO64) == 0u && p->reserved0 == 0u && p->base_time < kMp4TimeLimit && p->data_offset < kMp4TimeLimit;
}

#ifdef __HIPCC__
struct StblwArgs {
    StblwIn in;                           /* the samples' tables and the parameters their rules read                                */
    bool co64;
    uint32_t max_chunk;
    uint8_t* out; uint64_t out_cap;       /* out NULL: plan only                                                                    */
    hbs_mp4_stbl* tables;                 /* nullable                                                                               */
    hbs_summary* summary;
    /* scratch (lay_mp4stblw) */
    unsigned long long* last;             /* per sample block: 1 + its last sample that is not contiguous; then the maximum in front */
    unsigned long long* part_r;           /* 8 per sample block: chunk starts, stts runs, ctts runs, sync samples, 1 + the lowest bad
                                             sample                                                                                 */
    unsigned long long* part_s;           /* 8 per sample block: sample bytes, deltas, sizes other than the first, negative cts       */
    unsigned long long* part_c;           /* 8 per chunk block: stsc entries that begin in it                                         */
    unsigned long long* ctl;              /* 32 words: see hbs_mp4stblw.hip                                                                */
    unsigned long long* chunk_first;      /* n: the first sample of chunk c                                                          */
    unsigned long long* stts_first;       /* n: the first sample of stts entry t                                                     */
    unsigned long long* ctts_first;       /* n: the first sample of ctts entry j                                                     */
    hipEvent_t ev_begin, ev_end;
};

inline uint64_t stblw_blocks(uint64_t n) { return (n + kSwLanes - 1) / kSwLanes; }

/* scratch, by n_samples alone: 8 bytes a sample for the chunks' first samples and 8 each for those of the stts and ctts runs,
 * 200 bytes per 256 samples, 256 bytes */
inline void lay_mp4stblw(Carver& w, StblwArgs& a)
{
    const uint64_t kb = stblw_blocks(a.in.n);
    a.last = w.take<unsigned long long>(kb * 8);
    a.part_r = w.take<unsigned long long>(kb * 64);
    a.part_s = w.take<unsigned long long>(kb * 64);
    a.part_c = w.take<unsigned long long>(kb * 64);
    a.ctl = w.take<unsigned long long>(256);
    a.chunk_first = w.take<unsigned long long>(a.in.n * 8);
    a.stts_first = w.take<unsigned long long>(a.in.n * 8);
    a.ctts_first = w.take<unsigned long long>(a.in.n * 8);
}
hipError_t launch_mp4_stbl_write(const StblwArgs& a, hipStream_t st);
#endif

} // namespace hbs
#endif
