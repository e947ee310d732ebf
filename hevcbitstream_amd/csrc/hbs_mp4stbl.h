/*
 * hbs_mp4stbl.h -- hbs_mp4_stbl_samples and hbs_mp4_stbl_find_host (include/hevcbitstream_amd.h): the rules that read the
 * sample table (stbl) of a progressive MP4 (ISO/IEC 14496-12) as host/device inline functions -- stbl_heads decodes the six
 * boxes' fixed parts and checks versions and lengths, stbl_stsc_entry / stbl_stss_entry check one entry against its
 * neighbour, stbl_run_samples / stbl_join keep the sums exact where counts of 2^32 - 1 meet, stbl_place checks a sample's
 * offset and times; the kernels of hbs_mp4stbl.hip, the host checks and the tests all run them -- the box finder and the track
 * reader (plain host code, no GPU; their walk is mp4rd_find_track of hbs_mp4rd.h, whose Mp4TrackPath names the stbl), and the
 * host-visible launcher.  Everything above the launcher compiles with plain g++.
 */
#ifndef HBS_MP4STBL_H
#define HBS_MP4STBL_H

#include "hbs_mp4rd.h"

namespace hbs {

constexpr int kStLanes = 256;                        /* lanes of a workgroup: a table entry or a sample a lane                   */
constexpr uint64_t kStMany = 1ull << 32;             /* a run's samples are counted up to this: more than any N                  */
enum : int { kStsz = 0, kStco = 1, kStsc = 2, kStts = 3, kCtts = 4, kStss = 5, kStBoxes = 6 };   /* the order of the errors  */

struct StblBox { uint64_t off, bytes; };             /* the payload behind the box header; bytes == 0: no such box               */

/* what the six payloads' fixed parts say; a box that is broken (or absent) has count 0 */
struct StblHead {
    uint64_t N, C, E, T, K, S;       /* samples, chunks, the entries of stsc, stts, ctts, stss                                  */
    uint32_t ssz;                    /* stsz: the constant sample size, 0: a table                                              */
    uint32_t ctts_v;                 /* ctts: its version                                                                       */
    uint32_t bad;                    /* 1 + the first box whose version or length is wrong; 0: none                              */
};

/* the fixed part of one full box: version/flags(4), `fixed` - 8 further bytes, count(4); `entry` bytes a count.  false: the
 * version is above max_version, or the payload is shorter than fixed + count x entry */
HBS_HD bool stbl_counted(const uint8_t* p, const StblBox& b, uint32_t fixed, uint32_t entry, uint32_t max_version, uint64_t& count, uint32_t& version)
{
    count = 0; version = 0;
    if (b.bytes < fixed) return false;
    version = rd_be32(p, b.off) >> 24;
    if (version > max_version) return false;
    const uint64_t c = rd_be32(p, b.off + fixed - 4u);
    if (entry && c > (b.bytes - fixed) / entry) return false;
    count = c;
    return true;
}

HBS_HD void stbl_heads(const uint8_t* p, const StblBox box[kStBoxes], bool co64, StblHead& h)
{
    uint32_t v;
    h.N = 0; h.C = 0; h.E = 0; h.T = 0; h.K = 0; h.S = 0; h.ssz = 0; h.ctts_v = 0; h.bad = 0;
    /* stsz: sample_size(4) count(4), then count sizes iff sample_size == 0 */
    bool ok = box[kStsz].bytes >= 12u;
    if (ok) { h.ssz = rd_be32(p, box[kStsz].off + 4u); ok = stbl_counted(p, box[kStsz], 12u, h.ssz ? 0u : 4u, 0u, h.N, v); }
    if (!ok) { h.bad = 1u + kStsz; h.ssz = 0; }
    if (!stbl_counted(p, box[kStco], 8u, co64 ? 8u : 4u, 0u, h.C, v) && !h.bad) h.bad = 1u + kStco;
    if (!stbl_counted(p, box[kStsc], 8u, 12u, 0u, h.E, v) && !h.bad) h.bad = 1u + kStsc;
    if (!stbl_counted(p, box[kStts], 8u, 8u, 0u, h.T, v) && !h.bad) h.bad = 1u + kStts;
    if (box[kCtts].bytes && !stbl_counted(p, box[kCtts], 8u, 8u, 1u, h.K, h.ctts_v) && !h.bad) h.bad = 1u + kCtts;
    if (box[kStss].bytes && !stbl_counted(p, box[kStss], 8u, 4u, 0u, h.S, v) && !h.bad) h.bad = 1u + kStss;
}

/* stsc entry e of E (C chunks): first_chunk is 1 in entry 0, strictly increasing and at most C.  chunks: those it covers, up to
 * the next entry's first_chunk, the last entry up to C.  false: it breaks the rule */
HBS_HD bool stbl_stsc_entry(const uint8_t* p, uint64_t entries, uint64_t e, uint64_t E, uint64_t C, uint32_t& first_chunk, uint32_t& per_chunk,
                            uint64_t& chunks)
{
    const uint64_t at = entries + e * 12u;
    first_chunk = rd_be32(p, at); per_chunk = rd_be32(p, at + 4u);
    chunks = 0;
    if (e == 0 ? first_chunk != 1u : first_chunk <= rd_be32(p, at - 12u)) return false;
    if (first_chunk > C) return false;
    const uint64_t next = e + 1u < E ? (uint64_t)rd_be32(p, at + 12u) : C + 1u;
    if (next <= first_chunk) return e + 1u < E;                /* (the next entry's lane reports it; this one covers nothing) */
    chunks = (next <= C + 1u ? next : C + 1u) - first_chunk;
    return true;
}

/* the samples of a run of `chunks` chunks of per_chunk samples, counted up to kStMany (both factors are below 2^32, so the
 * product is exact): sums of 2^32 - 1 such numbers stay below 2^64, and what lies at or above kStMany lies above every N */
HBS_HD uint64_t stbl_run_samples(uint64_t chunks, uint32_t per_chunk)
{
    const uint64_t s = chunks * per_chunk;
    return s < kStMany ? s : kStMany;
}

/* stss entry i: the sample numbers are strictly increasing and none is 0 */
HBS_HD bool stbl_stss_entry(const uint8_t* p, uint64_t entries, uint64_t i, uint32_t& number)
{
    number = rd_be32(p, entries + i * 4u);
    return number != 0u && (i == 0 || rd_be32(p, entries + i * 4u - 4u) < number);
}

/* The time at which an stts entry begins is the sum of count x delta over the entries in front of it; a product is below 2^64,
 * the sum of 2^32 - 1 of them is not.  So two sums are kept, of the products' high and low 32 bits (each below 2^64 for any
 * table), and joined here: the time, or kMp4TimeLimit when it is that or more. */
HBS_HD uint64_t stbl_join(uint64_t hi_sum, uint64_t lo_sum)
{
    if (hi_sum >= (kMp4TimeLimit >> 32) || lo_sum >= kMp4TimeLimit) return kMp4TimeLimit;
    const uint64_t t = (hi_sum << 32) + lo_sum;
    return t < kMp4TimeLimit ? t : kMp4TimeLimit;
}

/* where and when a sample is: its chunk's offset, the sizes of the chunk's earlier samples (below 2^64: 2^32 sizes of 32 bits),
 * its size, the bytes of the file; the time at which its stts entry begins (stbl_join), its place r in the entry, the entry's
 * delta, its composition offset.  false: a sample error (off, dts, pts mean nothing) */
HBS_HD bool stbl_place(uint64_t chunk_off, uint64_t before, uint32_t size, uint64_t file_bytes, uint64_t entry_time, uint64_t r, uint32_t delta,
                       int64_t cts, uint64_t& off, uint64_t& dts, uint64_t& pts)
{
    off = 0; dts = 0; pts = 0;
    if (chunk_off > file_bytes) return false;
    uint64_t room = file_bytes - chunk_off;
    if (before > room) return false;
    room -= before;
    if (size > room) return false;
    off = chunk_off + before;
    const uint64_t step = r * delta;                           /* (r < 2^32) */
    if (entry_time >= kMp4TimeLimit || step >= kMp4TimeLimit || entry_time + step >= kMp4TimeLimit) return false;
    dts = entry_time + step;
    const int64_t t = (int64_t)dts + cts;                      /* (|cts| < 2^32) */
    if (t < 0 || (uint64_t)t >= kMp4TimeLimit) return false;
    pts = (uint64_t)t;
    return true;
}

HBS_HD int64_t stbl_cts(uint32_t word, uint32_t version) { return version ? (int64_t)(int32_t)word : (int64_t)word; }

/* ---- host side --------------------------------------------------------------------------------------------------------- */

inline bool mp4_stbl_ok(const hbs_mp4_stbl* t)
{
    return t && (t->flags & ~(uint32_t)HBS_MP4_STBL_CO64) == 0u && t->reserved0 == 0u && t->reserved[0] == 0u && t->reserved[1] == 0u;
}

/* hbs_mp4_track_read_host: what hbs_mp4_init_read_host reads of the track, from a moov that needs no mvex: the trex fields are 0 */
inline int64_t mp4_track_read_host(const uint8_t* seg, uint64_t n, uint32_t track_id, hbs_mp4_track* out, uint64_t* nal_off, uint64_t* nal_bytes,
                                   uint64_t cap)
{
    if (!seg || !out || n > kRdMaxIn || (cap && (!nal_off || !nal_bytes))) return HBS_E_ARG;
    hbs_mp4_track t;
    Mp4TrackPath path;
    int64_t n_nals = -1;
    if (!mp4rd_find_track(seg, n, track_id, t, path, n_nals, nal_off, nal_bytes, cap)) return HBS_E_ARG;
    t.n_nals = (uint32_t)n_nals;
    *out = t;
    return n_nals;
}

inline int mp4_stbl_find_host(const uint8_t* seg, uint64_t n, uint64_t base, uint32_t track_id, hbs_mp4_stbl* out)
{
    if (!seg || !out || n > kRdMaxIn) return HBS_E_ARG;
    hbs_mp4_track t;
    Mp4TrackPath path;
    int64_t n_nals = -1;
    if (!mp4rd_find_track(seg, n, track_id, t, path, n_nals, nullptr, nullptr, 0)) return HBS_E_ARG;
    hbs_mp4_stbl r;
    memset(&r, 0, sizeof(r));
    bool stz2 = false, co64 = false;
    for (uint64_t at = path.box[kPathStbl].pay(), se = path.box[kPathStbl].end(); at < se;) {     /* (the chain held in the walk) */
        Mp4Box b;
        if (!mp4rd_box(seg, at, se, b)) return HBS_E_ARG;
        hbs_mp4_box_ref* ref = nullptr;
        bool is64 = false;
        switch (b.type) {
        case HBS_MP4_FOURCC('s', 't', 's', 'z'): ref = &r.stsz; break;
        case HBS_MP4_FOURCC('s', 't', 'c', 'o'): ref = &r.stco; break;
        case HBS_MP4_FOURCC('c', 'o', '6', '4'): ref = &r.stco; is64 = true; break;
        case HBS_MP4_FOURCC('s', 't', 's', 'c'): ref = &r.stsc; break;
        case HBS_MP4_FOURCC('s', 't', 't', 's'): ref = &r.stts; break;
        case HBS_MP4_FOURCC('c', 't', 't', 's'): ref = &r.ctts; break;
        case HBS_MP4_FOURCC('s', 't', 's', 's'): ref = &r.stss; break;
        case HBS_MP4_FOURCC('s', 't', 'z', '2'): stz2 = true; break;
        default: break;
        }
        /* the first of a type is used (of stco and co64: whichever comes first); bytes == 0 says "absent", so a table box
         * without a payload, which holds not even its version, is refused here */
        if (ref && ref->bytes == 0) {
            if (b.size == b.head) return HBS_E_ARG;
            ref->off = at + b.head + base; ref->bytes = b.size - b.head;
            if (ref == &r.stco) co64 = is64;
        }
        at += b.size;
    }
    (void)stz2;                                                /* (a stz2 without a stsz: no stsz, refused below) */
    if (!r.stsz.bytes || !r.stsc.bytes || !r.stts.bytes || !r.stco.bytes) return HBS_E_ARG;
    r.flags = co64 ? (uint32_t)HBS_MP4_STBL_CO64 : 0u;
    *out = r;
    return 0;
}

#ifdef __HIPCC__
struct StblArgs {
    const uint8_t* src; uint64_t n, file_bytes;
    StblBox box[kStBoxes]; bool co64;
    uint64_t cap[kStBoxes];           /* the entries each payload has bytes for (stsz: as a table), 2^32 - 1 at most               */
    uint64_t sample_cap;
    bool out;                         /* false: plan only                                                                         */
    unsigned long long* sample_off; unsigned long long* sample_size; unsigned long long* dts; unsigned long long* pts;
    uint32_t* sample_flags; hbs_summary* summary;
    /* scratch (lay_mp4stbl) */
    unsigned long long* part_r;       /* 8 per entry block: samples of the stsc runs, stts counts, the times' high and low sums,
                                         ctts counts, 1 + the first box with a broken entry                                       */
    unsigned long long* part_k;       /* 8 per sample block: the sizes' open sum, whether a chunk began                            */
    unsigned long long* part_c;       /* 8 per sample block (plan only: per stsz block): sample bytes, 1 + the lowest bad sample   */
    unsigned long long* ctl;          /* 16: see hbs_mp4stbl.hip                                                                  */
    unsigned long long* stsc_first;   /* cap[kStsc]: the run's first sample (with outputs)                                         */
    unsigned long long* stts_first;   /* cap[kStts]: the entry's first sample                                                      */
    unsigned long long* stts_time;    /* cap[kStts]: the time at which it begins (stbl_join)                                       */
    unsigned long long* ctts_first;   /* cap[kCtts]: the entry's first sample                                                      */
    hipEvent_t ev_begin, ev_end;
};

inline uint64_t stbl_entry_blocks(const StblArgs& a)
{
    uint64_t m = 0;
    for (int b = kStsc; b < kStBoxes; ++b) if (a.cap[b] > m) m = a.cap[b];
    return (m + kStLanes - 1) / kStLanes;
}

/* scratch: 64 bytes per 256 entries of the longest of stsc / stts / ctts / stss; plan only 64 bytes per 256 sizes of the stsz;
 * with outputs 8 bytes an entry of stsc and ctts, 16 an entry of stts, and 128 bytes per 256 samples of sample_cap */
inline void lay_mp4stbl(Carver& w, StblArgs& a)
{
    const uint64_t eb = stbl_entry_blocks(a);
    const uint64_t kb = a.out ? (a.sample_cap + kStLanes - 1) / kStLanes : 0;
    const uint64_t zb = a.out ? 0 : (a.cap[kStsz] + kStLanes - 1) / kStLanes;
    a.part_r = w.take<unsigned long long>(eb * 64);
    a.part_k = w.take<unsigned long long>(kb * 64);
    a.part_c = w.take<unsigned long long>((kb + zb) * 64);
    a.ctl = w.take<unsigned long long>(128);
    a.stsc_first = w.take<unsigned long long>(a.out ? a.cap[kStsc] * 8 : 0);
    a.stts_first = w.take<unsigned long long>(a.out ? a.cap[kStts] * 8 : 0);
    a.stts_time = w.take<unsigned long long>(a.out ? a.cap[kStts] * 8 : 0);
    a.ctts_first = w.take<unsigned long long>(a.out ? a.cap[kCtts] * 8 : 0);
}
hipError_t launch_mp4_stbl_samples(const StblArgs& a, hipStream_t st);
#endif

} // namespace hbs
#endif
