/*
 * hbs_mp4rd.h -- hbs_mp4_samples and hbs_mp4_init_read_host (include/hevcbitstream_amd.h): the rules that read fragmented MP4
 * (ISO/IEC 14496-12) as host/device inline functions -- mp4rd_tfhd and mp4rd_trun lay the optional fields out from the
 * flags, mp4rd_moof walks one moof and hands out its trun records, mp4rd_sample resolves an entry through the three levels of
 * defaults, mp4rd_place checks a sample's offset and times (the byte reads and the box rule are hbs_mp4box.h's); the kernels
 * of hbs_mp4rd.hip, the host checks and the tests all run them -- the init segment's reader (plain host code, no GPU: over the
 * walk of hbs_mp4box.h, mp4rd_find_track returns the track and its Mp4TrackPath, from which hbs_mp4stbl.h and hbs_mp4prot.h
 * take their boxes), and the host-visible launcher.  Everything above the launcher compiles with plain g++.
 */
#ifndef HBS_MP4RD_H
#define HBS_MP4RD_H

#include <string.h>
#include "hbs_mp4.h"

namespace hbs {

constexpr int kRdLanes = 256;                        /* lanes of a workgroup: a segment, a moof or a sample a lane             */
constexpr uint64_t kRdMaxIn = 1ull << 62;            /* in_bytes above this is refused: offsets stay inside an int64           */
constexpr uint64_t kRdBaseCap = (1ull << 62) + (1ull << 32);   /* a base_data_offset above this is taken as this: every sample
                                                                  behind it lies outside the buffer either way               */
constexpr uint64_t kRdLarge = 1ull << 63;            /* Mp4RdArgs.moof_size: the moof has a largesize (a size is 2^62 at most)   */
constexpr uint32_t kRdHead = 1u << 30;               /* Mp4TrunRec.tr: the sizes' sum restarts at the trun's first sample      */
constexpr uint32_t kRdMoofFirst = 1u << 31;          /* ... the durations' sum does: the moof's first sample                   */

struct Mp4Tfhd { uint32_t flags, track_id, dur, size, sflags; uint64_t base_data_offset; };

HBS_HD uint32_t mp4rd_tfhd_bytes(uint32_t flags)
{
    return 8u + ((flags & 1u) ? 8u : 0u) + ((flags & 2u) ? 4u : 0u) + ((flags & 8u) ? 4u : 0u) + ((flags & 0x10u) ? 4u : 0u) + ((flags & 0x20u) ? 4u : 0u);
}

/* the tfhd whose payload (behind the box header) is p[pay, pay + len); the version is not looked at */
HBS_HD bool mp4rd_tfhd(const uint8_t* p, uint64_t pay, uint64_t len, Mp4Tfhd& t)
{
    if (len < 8) return false;
    t.flags = rd_be32(p, pay) & 0xFFFFFFu; t.track_id = rd_be32(p, pay + 4);
    t.base_data_offset = 0; t.dur = 0; t.size = 0; t.sflags = 0;
    if (len < mp4rd_tfhd_bytes(t.flags)) return false;
    uint64_t q = pay + 8;
    if (t.flags & 1u) { t.base_data_offset = rd_be64(p, q); q += 8; }
    if (t.flags & 2u) q += 4;
    if (t.flags & 8u) { t.dur = rd_be32(p, q); q += 4; }
    if (t.flags & 0x10u) { t.size = rd_be32(p, q); q += 4; }
    if (t.flags & 0x20u) t.sflags = rd_be32(p, q);
    return true;
}

/* the tfdt with that payload */
HBS_HD bool mp4rd_tfdt(const uint8_t* p, uint64_t pay, uint64_t len, uint64_t& time)
{
    if (len < 4) return false;
    const uint32_t v = rd_be32(p, pay) >> 24;
    if (v > 1u || len < (v ? 12u : 8u)) return false;
    time = v ? rd_be64(p, pay + 4) : rd_be32(p, pay + 4);
    return true;
}

/* the mfhd with that payload */
HBS_HD bool mp4rd_mfhd(const uint8_t* p, uint64_t pay, uint64_t len, uint32_t& sequence)
{
    if (len < 8 || (rd_be32(p, pay) >> 24) != 0u) return false;
    sequence = rd_be32(p, pay + 4);
    return true;
}

HBS_HD uint32_t mp4rd_popc4(uint32_t nib) { return (nib & 1u) + ((nib >> 1) & 1u) + ((nib >> 2) & 1u) + ((nib >> 3) & 1u); }
/* bytes of one trun entry; the byte offset in it of the field `bit` (0x100 duration, 0x200 size, 0x400 flags, 0x800 cts) */
HBS_HD uint32_t mp4rd_entry_bytes(uint32_t flags) { return 4u * mp4rd_popc4((flags >> 8) & 0xFu); }
HBS_HD uint32_t mp4rd_field_at(uint32_t flags, uint32_t bit) { return 4u * mp4rd_popc4((flags >> 8) & 0xFu & ((bit >> 8) - 1u)); }

struct Mp4Trun { uint32_t flags, version, count, first_flags; int32_t data_offset; uint64_t entries; };

/* the trun with that payload: 8 + 4 [0x001] + 4 [0x004] + count x entry bytes must lie in it; entries: where they begin in p */
HBS_HD bool mp4rd_trun(const uint8_t* p, uint64_t pay, uint64_t len, Mp4Trun& t)
{
    if (len < 8) return false;
    const uint32_t vf = rd_be32(p, pay);
    t.version = vf >> 24; t.flags = vf & 0xFFFFFFu; t.count = rd_be32(p, pay + 4);
    t.data_offset = 0; t.first_flags = 0;
    if (t.version > 1u) return false;
    const uint64_t fixed = 8u + ((t.flags & 1u) ? 4u : 0u) + ((t.flags & 4u) ? 4u : 0u);
    if (len < fixed || (uint64_t)t.count * mp4rd_entry_bytes(t.flags) > len - fixed) return false;
    uint64_t q = pay + 8;
    if (t.flags & 1u) { t.data_offset = (int32_t)rd_be32(p, q); q += 4; }
    if (t.flags & 4u) { t.first_flags = rd_be32(p, q); q += 4; }
    t.entries = q;
    return true;
}

/* ---- one moof ---------------------------------------------------------------------------------------------------------- */

/* What a sample's lane needs of its trun (a trun of count 0 leaves none): 64 bytes. */
struct Mp4TrunRec {
    uint64_t entries;              /* the entry array's offset in the buffer                                              */
    int64_t begin;                 /* the data begin of the trun at which the sizes' sum last restarted (this one: kRdHead) */
    uint64_t tfdt;
    uint32_t first;                /* its first sample: within the moof from mp4rd_moof, within the call in the scratch     */
    uint32_t count;
    uint32_t tr;                   /* the trun's flags | version << 24 | kRdHead | kRdMoofFirst                            */
    uint32_t first_flags;
    uint32_t def_dur, def_size, def_flags;    /* the tfhd's, else the trex's                                              */
    uint32_t moof;
    uint32_t pad[2];
};

struct Mp4Moof { uint64_t tfdt, samples, truns; uint32_t sequence; };
struct Mp4Trex { uint32_t track_id, dur, size, flags; };

/* Walks the moof p[at, at + size) (header of `head` bytes) of the segment that begins at seg_off: emit(i, rec) for the i-th
 * trun with samples of the traf that is read.  false: a moof error. */
template <class Emit>
HBS_HD bool mp4rd_moof(const uint8_t* p, uint64_t seg_off, uint64_t at, uint64_t size, uint32_t head, const Mp4Trex& x, Mp4Moof& m, Emit&& emit)
{
    const uint64_t end = at + size;
    bool have_mfhd = false, found = false;
    uint32_t traf_i = 0;
    m.tfdt = 0; m.samples = 0; m.truns = 0; m.sequence = 0;
    for (uint64_t q = at + head; q < end;) {
        Mp4Box b;
        if (!mp4rd_box(p, q, end, b)) return false;
        if (b.type == HBS_MP4_FOURCC('m', 'f', 'h', 'd') && !have_mfhd) {
            if (!mp4rd_mfhd(p, q + b.head, b.size - b.head, m.sequence)) return false;
            have_mfhd = true;
        } else if (b.type == HBS_MP4_FOURCC('t', 'r', 'a', 'f') && !found) {
            const uint64_t t0 = q + b.head, tend = q + b.size;
            Mp4Tfhd h;
            bool have_tfhd = false, have_tfdt = false;
            uint64_t dt_pay = 0, dt_len = 0;
            for (uint64_t c = t0; c < tend;) {
                Mp4Box k;
                if (!mp4rd_box(p, c, tend, k)) return false;
                if (k.type == HBS_MP4_FOURCC('t', 'f', 'h', 'd') && !have_tfhd) {
                    if (!mp4rd_tfhd(p, c + k.head, k.size - k.head, h)) return false;
                    have_tfhd = true;
                } else if (k.type == HBS_MP4_FOURCC('t', 'f', 'd', 't') && !have_tfdt) {
                    dt_pay = c + k.head; dt_len = k.size - k.head; have_tfdt = true;
                }
                c += k.size;
            }
            if (!have_tfhd) return false;
            if (x.track_id == 0u || h.track_id == x.track_id) {
                found = true;
                if (!have_tfdt || !mp4rd_tfdt(p, dt_pay, dt_len, m.tfdt)) return false;
                int64_t base;
                if (h.flags & 1u) base = (int64_t)(seg_off + (h.base_data_offset < kRdBaseCap ? h.base_data_offset : kRdBaseCap));
                else if ((h.flags & 0x020000u) || traf_i == 0u) base = (int64_t)at;
                else return false;
                Mp4TrunRec r;
                r.tfdt = m.tfdt; r.moof = 0; r.pad[0] = 0; r.pad[1] = 0;
                r.def_dur = (h.flags & 8u) ? h.dur : x.dur;
                r.def_size = (h.flags & 0x10u) ? h.size : x.size;
                r.def_flags = (h.flags & 0x20u) ? h.sflags : x.flags;
                bool pending = true;
                int64_t pend = base, chain = base;
                for (uint64_t c = t0; c < tend;) {
                    Mp4Box k;
                    (void)mp4rd_box(p, c, tend, k);                    /* (it held above) */
                    if (k.type == HBS_MP4_FOURCC('t', 'r', 'u', 'n')) {
                        Mp4Trun t;
                        if (!mp4rd_trun(p, c + k.head, k.size - k.head, t)) return false;
                        if (t.flags & 1u) { pending = true; pend = base + t.data_offset; }
                        if (t.count) {
                            if (pending) chain = pend;
                            r.entries = t.entries; r.begin = chain; r.count = t.count; r.first_flags = t.first_flags;
                            r.first = (uint32_t)m.samples;
                            r.tr = (t.flags & 0xFFFu) | (t.version << 24) | (pending ? kRdHead : 0u) | (m.samples == 0 ? kRdMoofFirst : 0u);
                            pending = false;
                            emit(m.truns, r);
                            m.truns += 1; m.samples += t.count;
                        }
                    }
                    c += k.size;
                }
            }
            traf_i += 1;
        } else if (b.type == HBS_MP4_FOURCC('t', 'r', 'a', 'f')) traf_i += 1;
        q += b.size;
    }
    return have_mfhd;
}

/* ---- one sample -------------------------------------------------------------------------------------------------------- */

struct Mp4Sample { uint32_t dur, size, flags; int64_t cts; };

/* entry e of the trun: each field the entry's, else first_sample_flags (flags of entry 0 of a trun with 0x004), else the default */
HBS_HD Mp4Sample mp4rd_sample(const uint8_t* p, const Mp4TrunRec& t, uint32_t e)
{
    const uint64_t at = t.entries + (uint64_t)e * mp4rd_entry_bytes(t.tr);
    Mp4Sample s;
    s.dur = (t.tr & 0x100u) ? rd_be32(p, at) : t.def_dur;
    s.size = (t.tr & 0x200u) ? rd_be32(p, at + mp4rd_field_at(t.tr, 0x200u)) : t.def_size;
    s.flags = (t.tr & 0x400u) ? rd_be32(p, at + mp4rd_field_at(t.tr, 0x400u)) : (e == 0u && (t.tr & 4u)) ? t.first_flags : t.def_flags;
    s.cts = 0;
    if (t.tr & 0x800u) {
        const uint32_t c = rd_be32(p, at + mp4rd_field_at(t.tr, 0x800u));
        s.cts = ((t.tr >> 24) & 1u) ? (int64_t)(int32_t)c : (int64_t)c;
    }
    return s;
}

HBS_HD bool mp4rd_sync(uint32_t sample_flags) { return (sample_flags & 0x00010000u) == 0u; }

/* where and when a sample is: its trun chain's data begin, the sizes in front of it in the chain, its size; its moof's tfdt,
 * the durations in front of it in the moof, its composition offset.  false: a sample error (off, dts, pts mean nothing) */
HBS_HD bool mp4rd_place(int64_t begin, uint64_t before, uint32_t size, uint64_t in_bytes, uint64_t tfdt, uint64_t dur_before, int64_t cts,
                        uint64_t& off, uint64_t& dts, uint64_t& pts)
{
    off = 0; dts = 0; pts = 0;
    if (begin < 0 || (uint64_t)begin > in_bytes) return false;
    uint64_t room = in_bytes - (uint64_t)begin;
    if (before > room) return false;
    room -= before;
    if (size > room) return false;
    off = (uint64_t)begin + before;
    if (tfdt >= kMp4TimeLimit || dur_before >= kMp4TimeLimit || tfdt + dur_before >= kMp4TimeLimit) return false;
    dts = tfdt + dur_before;
    const int64_t t = (int64_t)dts + cts;                  /* (|cts| < 2^32) */
    if (t < 0 || (uint64_t)t >= kMp4TimeLimit) return false;
    pts = (uint64_t)t;
    return true;
}

/* A trun whose entries have no bytes is `count` samples of the default size and duration with no composition offset: sample e
 * lies at begin + before + e x size and has dts = pts = tfdt + dur_before + e x dur.  Both grow with e, so what mp4rd_place
 * would say of every sample follows from sample 0 and two divisions: returns how many samples in front of the lowest bad one
 * are good (count: all).  The count is bounded by nothing in the box -- 2^32 - 1 samples in 16 bytes -- so nothing may loop
 * over it. */
HBS_HD uint64_t mp4rd_run_good(int64_t begin, uint64_t before, uint32_t size, uint64_t in_bytes, uint64_t tfdt, uint64_t dur_before, uint32_t dur,
                               uint64_t count)
{
    uint64_t off, dts, pts;
    if (!mp4rd_place(begin, before, size, in_bytes, tfdt, dur_before, 0, off, dts, pts)) return 0;
    uint64_t good = count;
    if (size) {                                                /* e is good iff off + (e + 1) size <= in_bytes */
        const uint64_t fit = (in_bytes - off) / size;
        if (fit < good) good = fit;
    }
    if (dur) {                                                 /* ... and dts + e dur <= 2^62 - 1 */
        const uint64_t fit = (kMp4TimeLimit - 1u - dts) / dur + 1u;
        if (fit < good) good = fit;
    }
    return good;
}

/* ---- host side --------------------------------------------------------------------------------------------------------- */

inline bool mp4_read_params_ok(const hbs_mp4_read_params* p)
{
    return p && p->flags == 0u && p->reserved[0] == 0u && p->reserved[1] == 0u && p->reserved[2] == 0u;
}

/* the parameter-set NALs of the hvcC payload p[at, end): their number, or -1; offsets and sizes while they fit cap */
inline int64_t mp4rd_hvcc(const uint8_t* p, uint64_t at, uint64_t end, int32_t& length_size, uint64_t* nal_off, uint64_t* nal_bytes, uint64_t cap)
{
    if (end - at < 23 || p[at] != 1u) return -1;
    length_size = (int32_t)(p[at + 21] & 3u) + 1;
    const uint32_t arrays = p[at + 22];
    uint64_t q = at + 23, n = 0;
    for (uint32_t a = 0; a < arrays; ++a) {
        if (end - q < 3) return -1;
        const uint32_t count = ((uint32_t)p[q + 1] << 8) | p[q + 2];
        q += 3;
        for (uint32_t i = 0; i < count; ++i) {
            if (end - q < 2) return -1;
            const uint32_t len = ((uint32_t)p[q] << 8) | p[q + 1];
            q += 2;
            if (end - q < len) return -1;
            if (n < cap && nal_off && nal_bytes) { nal_off[n] = q; nal_bytes[n] = len; }
            n += 1; q += len;
        }
    }
    return (int64_t)n;
}

/* the trak path.box[kPathTrak]: 1 a video track with an hvcC (out's track fields and the NALs filled, path filled down to the
 * first 'hvc1' or 'hev1' entry that holds an hvcC), 0 not one, -1 malformed */
inline int mp4rd_trak(const uint8_t* p, Mp4TrackPath& path, hbs_mp4_track* out, int64_t& n_nals, uint64_t* nal_off, uint64_t* nal_bytes, uint64_t cap)
{
    const Mp4At& trak = path.box[kPathTrak];
    Mp4Tkhd k;
    if (!mp4_tkhd(p, trak.pay(), trak.end(), k)) return -1;
    out->track_id = k.track_id; out->width = k.width; out->height = k.height;
    const int rc = mp4_track_descend(p, path, true, [&](uint32_t type, const Mp4At& e) -> int {
        if (type != HBS_MP4_FOURCC('h', 'v', 'c', '1') && type != HBS_MP4_FOURCC('h', 'e', 'v', '1')) return 0;
        if (e.size - e.head < 78) return -1;                   /* a VisualSampleEntry's fixed part */
        Mp4At h;
        const int c = mp4_child(p, e.pay() + 78, e.end(), HBS_MP4_FOURCC('h', 'v', 'c', 'C'), h);
        if (c <= 0) return c;
        out->entry = type; out->hvcc_off = h.pay(); out->hvcc_bytes = h.size - h.head;
        n_nals = mp4rd_hvcc(p, h.pay(), h.end(), out->length_size, nal_off, nal_bytes, cap);
        return n_nals < 0 ? -1 : 1;
    });
    if (rc < 0) return -1;
    Mp4At m, mdia = path.box[kPathMdia];                       /* (the mdhd is required of every trak, one without a minf included) */
    if (mp4_child(p, mdia.pay(), mdia.end(), HBS_MP4_FOURCC('m', 'd', 'h', 'd'), m) <= 0 || m.size - m.head < 4) return -1;
    const uint32_t mv = p[m.pay()];
    if (mv > 1u || m.size - m.head < (mv ? 32u : 20u)) return -1;
    out->timescale = rd_be32(p, m.pay() + (mv ? 20u : 12u));
    return rc;
}

/* The walk that the five init-segment calls share: the moov of seg[0, n) and in it the trak asked for -- track_id, or with 0
 * the first that is a video track with an hvcC; the others are stepped over, but must be well-formed.  t and the NALs as
 * mp4rd_trak leaves them; path: the seven boxes from the moov to the track's sample entry. */
inline bool mp4rd_find_track(const uint8_t* seg, uint64_t n, uint32_t track_id, hbs_mp4_track& t, Mp4TrackPath& path, int64_t& n_nals,
                             uint64_t* nal_off, uint64_t* nal_bytes, uint64_t cap)
{
    Mp4TrackPath k;                                            /* the trak that is looked at */
    if (mp4_child(seg, 0, n, HBS_MP4_FOURCC('m', 'o', 'o', 'v'), k.box[kPathMoov]) <= 0) return false;
    const Mp4At moov = k.box[kPathMoov];
    n_nals = -1;
    bool found = false;
    for (uint64_t at = moov.pay(); at < moov.end();) {
        Mp4Box b;
        if (!mp4rd_box(seg, at, moov.end(), b)) return false;
        if (b.type == HBS_MP4_FOURCC('t', 'r', 'a', 'k') && !found) {
            hbs_mp4_track c;
            memset(&c, 0, sizeof(c));
            int64_t cn = -1;
            k.box[kPathTrak] = Mp4At{at, b.size, b.head};
            const int rc = mp4rd_trak(seg, k, &c, cn, nal_off, nal_bytes, cap);
            if (rc < 0) return false;
            /* the track asked for must be a video track with an hvcC; with track_id 0 the others are stepped over */
            if (track_id == 0u ? rc == 1 : c.track_id == track_id) {
                if (rc != 1) return false;
                found = true; n_nals = cn; t = c; path = k;
            }
        }
        at += b.size;
    }
    return found;
}

/* hbs_mp4_init_read_host; path_out (nullable): the seven boxes down to the track's sample entry, for mp4_init_protect */
inline int64_t mp4_init_read_host(const uint8_t* seg, uint64_t n, uint32_t track_id, hbs_mp4_track* out, uint64_t* nal_off, uint64_t* nal_bytes,
                                  uint64_t cap, Mp4TrackPath* path_out = nullptr)
{
    if (!seg || !out || n > kRdMaxIn || (cap && (!nal_off || !nal_bytes))) return HBS_E_ARG;
    hbs_mp4_track t;
    Mp4TrackPath path;
    int64_t n_nals = -1;
    if (!mp4rd_find_track(seg, n, track_id, t, path, n_nals, nal_off, nal_bytes, cap)) return HBS_E_ARG;
    const Mp4At& moov = path.box[kPathMoov];
    Mp4At x;
    if (mp4_child(seg, moov.pay(), moov.end(), HBS_MP4_FOURCC('m', 'v', 'e', 'x'), x) <= 0) return HBS_E_ARG;
    bool have_trex = false;
    for (uint64_t at = x.pay(); at < x.end();) {
        Mp4Box b;
        if (!mp4rd_box(seg, at, x.end(), b)) return HBS_E_ARG;
        if (b.type == HBS_MP4_FOURCC('t', 'r', 'e', 'x') && !have_trex) {
            const uint64_t a = at + b.head;
            if (b.size - b.head < 24) return HBS_E_ARG;
            if (rd_be32(seg, a + 4) == t.track_id) {
                t.trex_duration = rd_be32(seg, a + 12); t.trex_size = rd_be32(seg, a + 16); t.trex_flags = rd_be32(seg, a + 20);
                have_trex = true;
            }
        }
        at += b.size;
    }
    if (!have_trex) return HBS_E_ARG;
    t.n_nals = (uint32_t)n_nals;
    *out = t;
    if (path_out) *path_out = path;
    return n_nals;
}

#ifdef __HIPCC__
struct Mp4RdArgs {
    const uint8_t* src; uint64_t n;
    const uint8_t* seg; uint64_t seg_stride, n_segs;  /* seg NULL: one segment, the buffer (n_segs 1)                              */
    Mp4Trex x;
    uint64_t moof_cap, sample_cap;
    bool out;                                         /* false: plan only                                                          */
    unsigned long long* sample_off; unsigned long long* sample_size; unsigned long long* dts; unsigned long long* pts;
    uint32_t* sample_flags; hbs_mp4_frag* frag; hbs_summary* summary;
    /* scratch (lay_mp4rd) */
    unsigned long long* part_s;    /* 8 per segment block: moofs, 1 + the lowest segment with a chain error                        */
    unsigned long long* part_m;    /* 8 per moof block: truns with samples, samples, 1 + the lowest moof with a moof error          */
    unsigned long long* part_e;    /* 8 per moof block (plan only): sample bytes, -, 1 + the lowest sample with a sample error      */
    unsigned long long* part_k;    /* 8 per sample block: the sizes' and the durations' open sums, whether each restarted           */
    unsigned long long* part_c;    /* 8 per sample block: sample bytes, 1 + the lowest sample with a sample error                   */
    unsigned long long* ctl;       /* 8: error, moofs, samples, truns, bad segment, bad moof, stop (1: the moofs are not read, 2:
                                      the samples are not)                                                                         */
    unsigned long long* seg_cnt;   /* n_segs: the segment's moofs                                                                   */
    unsigned long long* moof_cnt;  /* 2 moof_cap: the moof's truns with samples, its samples                                        */
    unsigned long long* moof_at;   /* moof_cap: the moof's offset in the buffer                                                     */
    unsigned long long* moof_size; /* moof_cap: its box size, | kRdLarge when its header has 16 bytes                               */
    unsigned long long* moof_seg;  /* moof_cap: its segment's offset                                                                */
    unsigned long long* moof_span; /* moof_cap: the bytes from the moof to the next of its segment or the segment's end            */
    hbs_mp4_frag* frag_tmp;        /* moof_cap: d_frag's records, copied out by the last kernel                                     */
    Mp4TrunRec* trun;              /* sample_cap: the truns with samples                                                            */
    uint32_t* trun_first;          /* sample_cap + 1: their first samples (then the sample count)                                   */
    hipEvent_t ev_begin, ev_end;
};

/* scratch: 8 bytes a segment and 64 per 256 of them; 96 bytes a moof of moof_cap and 128 per 256 of them; with outputs 68 bytes
 * a sample of sample_cap (a trun that is kept has a sample or more) and 128 per 256 of them */
inline void lay_mp4rd(Carver& w, Mp4RdArgs& a)
{
    const uint64_t sb = (a.n_segs + kRdLanes - 1) / kRdLanes, mb = (a.moof_cap + kRdLanes - 1) / kRdLanes;
    const uint64_t kb = a.out ? (a.sample_cap + kRdLanes - 1) / kRdLanes : 0;
    a.part_s = w.take<unsigned long long>(sb * 64);
    a.part_m = w.take<unsigned long long>(mb * 64);
    a.part_e = w.take<unsigned long long>(mb * 64);
    a.part_k = w.take<unsigned long long>(kb * 64);
    a.part_c = w.take<unsigned long long>(kb * 64);
    a.ctl = w.take<unsigned long long>(64);
    a.seg_cnt = w.take<unsigned long long>(a.n_segs * 8);
    a.moof_cnt = w.take<unsigned long long>(a.moof_cap * 16);
    a.moof_at = w.take<unsigned long long>(a.moof_cap * 8);
    a.moof_size = w.take<unsigned long long>(a.moof_cap * 8);
    a.moof_seg = w.take<unsigned long long>(a.moof_cap * 8);
    a.moof_span = w.take<unsigned long long>(a.moof_cap * 8);
    a.frag_tmp = w.take<hbs_mp4_frag>(a.moof_cap * 48);
    a.trun = w.take<Mp4TrunRec>(a.out ? a.sample_cap * 64 : 0);
    a.trun_first = w.take<uint32_t>(a.out ? (a.sample_cap + 1) * 4 : 0);
}
hipError_t launch_mp4_samples(const Mp4RdArgs& a, hipStream_t st);
#endif

} // namespace hbs
#endif
