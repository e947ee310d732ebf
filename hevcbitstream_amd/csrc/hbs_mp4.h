/*
 * hbs_mp4.h -- hbs_mp4_fragment, hbs_mp4_init_host and hbs_mp4_moov_host (include/hevcbitstream_amd.h): the rule that lays
 * one fMP4 fragment (moof + mdat, ISO/IEC 14496-12) out, as host/device inline functions -- mp4_head_word gives every 32-bit
 * word of the container bytes in front of a fragment's samples, mp4_frag_byte the byte at a fragment-relative offset,
 * mp4_len_byte a byte of a record's length field; the copy kernel of hbs_mp4.hip, the host checks and the tests all run them --
 * the times' rule, the builder of the init segment and of a progressive file's moov (mp4_moov_build: plain host code, no GPU),
 * and the host-visible launcher.  Everything above the launcher compiles with plain g++.
 */
#ifndef HBS_MP4_H
#define HBS_MP4_H

#include "hbs_mp4box.h"

namespace hbs {

constexpr int kMp4Lanes = 256;                       /* plan: lanes of a workgroup ...                               */
constexpr int kMp4NalsPer = 1;                       /* ... NAL side: a NAL a lane                                   */
constexpr int kMp4NalsPerBlock = kMp4Lanes * kMp4NalsPer;
constexpr int kMp4AusPerBlock = kMp4Lanes;           /* ... AU side: an AU a lane                                    */
constexpr uint64_t kMp4TileBytes = 64 * 1024;        /* copy: output bytes of one workgroup                          */
constexpr uint64_t kMp4TimeLimit = 1ull << 62;       /* a time at or above this is an error                          */
constexpr uint32_t kMp4MoofHead = 88;                /* bytes of a fragment in front of its trun entries             */
constexpr uint32_t kMp4FragFixed = 96;               /* ... and with the mdat header: what a fragment adds to 16 S + P */
constexpr uint64_t kMp4MaxSamples = (0xFFFFFFFFull - kMp4MoofHead) / 16u;     /* 88 + 16 S is a 32-bit box size      */
constexpr uint64_t kMp4MaxPayload = 0xFFFFFFFFull - 8u;                       /* 8 + P too: there is no 64-bit mdat  */

HBS_HD uint64_t mp4_fragment_bytes(uint64_t samples, uint64_t sample_bytes) { return kMp4FragFixed + 16u * samples + sample_bytes; }

/* ---- times ------------------------------------------------------------------------------------------------------------- */

/* dts(a) without a d_dts: base_time + a * sample_duration, exactly; false when that is 2^62 or more (base_time is below 2^62,
 * both factors below 2^32) */
HBS_HD bool mp4_ruled_dts(uint64_t base_time, uint64_t a, uint32_t sample_duration, uint64_t& t)
{
    const uint64_t prod = a * (uint64_t)sample_duration;
    t = base_time + prod;                                  /* (below 2^65 - 2^33 + 2^62: may wrap, so test first) */
    return prod <= kMp4TimeLimit - 1u - base_time;
}

/* the time rules of AU a, given its dts, the next AU's (last: this is the call's last AU) and its pts (have_pts); dur and cts
 * are the trun entry's two time words */
HBS_HD bool mp4_au_times(uint64_t dts, bool dts_ok, bool last, uint64_t next_dts, uint32_t sample_duration, bool have_pts, uint64_t pts,
                         uint32_t& dur, uint32_t& cts)
{
    dur = sample_duration; cts = 0;
    if (!dts_ok || dts >= kMp4TimeLimit) return false;
    if (!last) {
        if (next_dts < dts || next_dts - dts > 0xFFFFFFFFull) return false;
        dur = (uint32_t)(next_dts - dts);
    }
    if (have_pts) {
        if (pts >= kMp4TimeLimit) return false;
        const int64_t d = (int64_t)pts - (int64_t)dts;
        if (d < -2147483648ll || d > 2147483647ll) return false;
        cts = (uint32_t)(int32_t)d;
    }
    return true;
}

HBS_HD uint32_t mp4_sample_flags(bool irap) { return irap ? 0x02000000u : 0x01010000u; }

/* ---- the bytes of a fragment --------------------------------------------------------------------------------------------- */

/* 32-bit word w (big-endian in the output) of fragment f's container bytes: w < 22 the moof up to the trun entries, w = 22 and
 * 23 the mdat header (which lies behind the 4 S words of the entries) */
HBS_HD uint32_t mp4_head_word(const hbs_mp4_frag& f, uint32_t track_id, uint32_t w)
{
    const uint32_t s16 = 16u * f.samples;
    switch (w) {
    case 0:  return kMp4MoofHead + s16;
    case 1:  return HBS_MP4_FOURCC('m', 'o', 'o', 'f');
    case 2:  return 16u;
    case 3:  return HBS_MP4_FOURCC('m', 'f', 'h', 'd');
    case 4:  return 0u;
    case 5:  return f.sequence;
    case 6:  return 64u + s16;
    case 7:  return HBS_MP4_FOURCC('t', 'r', 'a', 'f');
    case 8:  return 16u;
    case 9:  return HBS_MP4_FOURCC('t', 'f', 'h', 'd');
    case 10: return 0x00020000u;
    case 11: return track_id;
    case 12: return 20u;
    case 13: return HBS_MP4_FOURCC('t', 'f', 'd', 't');
    case 14: return 0x01000000u;
    case 15: return (uint32_t)(f.decode_time >> 32);
    case 16: return (uint32_t)f.decode_time;
    case 17: return 20u + s16;
    case 18: return HBS_MP4_FOURCC('t', 'r', 'u', 'n');
    case 19: return 0x01000F01u;
    case 20: return f.samples;
    case 21: return kMp4FragFixed + s16;
    case 22: return (uint32_t)(f.out_bytes - (kMp4MoofHead + s16));          /* 8 + P */
    default: return HBS_MP4_FOURCC('m', 'd', 'a', 't');
    }
}

/* what byte m of a fragment's container bytes, m < 96 + 16 S, is made from: false: word w of mp4_head_word; true: word `w`
 * (0 duration, 1 size, 2 flags, 3 composition offset) of the trun entry of the fragment's sample `e` */
HBS_HD bool mp4_head_place(uint32_t samples, uint64_t m, uint32_t& w, uint32_t& e)
{
    const uint64_t q = m >> 2;
    e = 0;
    if (q < 22u) { w = (uint32_t)q; return false; }
    if (q < 22u + 4ull * samples) { e = (uint32_t)((q - 22u) >> 2); w = (uint32_t)((q - 22u) & 3u); return true; }
    w = (uint32_t)(q - 4ull * samples);
    return false;
}

/* THE RULE: the byte at fragment-relative offset m, m < 96 + 16 S, given the fragment's record and the four words sw
 * (duration, size, flags, composition offset) of the sample whose trun entry holds m (unused elsewhere) */
HBS_HD uint32_t mp4_frag_byte(const hbs_mp4_frag& f, uint32_t track_id, const uint32_t sw[4], uint64_t m)
{
    uint32_t w, e;
    const uint32_t v = mp4_head_place(f.samples, m, w, e) ? sw[w] : mp4_head_word(f, track_id, w);
    return (v >> (8u * (3u - (uint32_t)(m & 3u)))) & 0xFFu;
}

/* byte i (0 .. L - 1) of the L-byte big-endian length field of a record of `len` payload bytes */
HBS_HD uint32_t mp4_len_byte(uint64_t len, uint32_t L, uint32_t i) { return (uint32_t)(len >> (8u * (L - 1u - i))) & 0xFFu; }
HBS_HD bool mp4_len_fits(uint64_t len, uint32_t L) { return L >= 8u || (len >> (8u * L)) == 0; }

/* ---- host side: parameters, one fragment, the init segment --------------------------------------------------------------- */

inline bool mp4_params_ok(const hbs_mp4_params* p)
{
    if (!p || (p->length_size != 1 && p->length_size != 2 && p->length_size != 4)) return false;
    return (p->flags & ~HBS_MP4_CUT_AT_IRAP) == 0 && p->track_id != 0 && p->base_time < kMp4TimeLimit;
}

/* One sample of mp4_write_fragment_host: its trun words and its records, already length-prefixed (size bytes). */
struct Mp4HostSample { uint32_t sw[4]; const uint8_t* bytes; };

/* the fragment f of the samples s[0, f.samples) into out[0, f.out_bytes): the container bytes through the rule, byte by byte,
 * then the samples */
inline void mp4_write_fragment_host(const hbs_mp4_frag& f, uint32_t track_id, const Mp4HostSample* s, uint8_t* out)
{
    const uint64_t head = kMp4FragFixed + 16ull * f.samples;
    const uint32_t none[4] = {0, 0, 0, 0};
    for (uint64_t m = 0; m < head; ++m) {
        uint32_t w, e;
        const bool entry = mp4_head_place(f.samples, m, w, e);
        out[m] = (uint8_t)mp4_frag_byte(f, track_id, entry ? s[e].sw : none, m);
    }
    uint64_t at = head;
    for (uint32_t e = 0; e < f.samples; ++e)
        for (uint32_t i = 0; i < s[e].sw[1]; ++i) out[at++] = s[e].bytes[i];
}

/* a writer that counts when it has no buffer */
struct Mp4Writer {
    uint8_t* p; uint64_t n;
    void u8(uint32_t v) { if (p) p[n] = (uint8_t)v; n += 1; }
    void u16(uint32_t v) { u8(v >> 8); u8(v); }
    void u32(uint32_t v) { u16(v >> 16); u16(v); }
    void zeros(uint32_t k) { for (uint32_t i = 0; i < k; ++i) u8(0); }
    void bytes(const uint8_t* b, uint64_t k) { for (uint64_t i = 0; i < k; ++i) u8(b[i]); }
    uint64_t box(uint32_t fourcc) { const uint64_t at = n; u32(0); u32(fourcc); return at; }
    uint64_t full(uint32_t fourcc, uint32_t flags) { const uint64_t at = box(fourcc); u32(flags & 0xFFFFFFu); return at; }
    void end(uint64_t at, uint64_t behind = 0)                  /* behind: bytes of the box that the caller appends later */
    {
        const uint64_t size = n - at + behind;
        if (p) wr_be32(p + at, (uint32_t)size);
    }
    void matrix() { u32(0x00010000u); zeros(12); u32(0x00010000u); zeros(12); u32(0x40000000u); }
};

/* the first `want` bytes of nal[0, n) with emulation prevention stripped (a 03 behind two zero bytes is dropped) into out;
 * returns how many there are (fewer when the NAL ends first).  Reads no byte at or behind nal + n. */
inline uint32_t mp4_strip_prefix(const uint8_t* nal, uint64_t n, uint8_t* out, uint32_t want)
{
    uint32_t got = 0, zeros = 0;
    for (uint64_t i = 0; i < n && got < want; ++i) {
        const uint8_t b = nal[i];
        if (zeros >= 2 && b == 3) { zeros = 0; continue; }
        zeros = b == 0 ? zeros + 1 : 0;
        out[got++] = b;
    }
    return got;
}

/* hbs_mp4_init_host (prog == nullptr) and hbs_mp4_moov_host share one builder: with a prog the times carry its duration, the
 * stbl ends behind the stsd, there is no mvex, and every box that holds the stbl counts prog->tables_bytes more than is written */
struct Mp4Prog { uint64_t duration, tables_bytes; };

inline int64_t mp4_moov_build(const hbs_mp4_init_params* p, int flags, const uint8_t* const* nal, const uint64_t* nal_bytes, uint64_t n,
                              const Mp4Prog* prog, uint8_t* out, uint64_t cap)
{
    if (prog && (prog->duration > 0xFFFFFFFFull || prog->tables_bytes % 4u != 0 || prog->tables_bytes > 0xFFFFFFFFull)) return HBS_E_ARG;
    const uint32_t dur = prog ? (uint32_t)prog->duration : 0u;
    const uint64_t tb = prog ? prog->tables_bytes : 0;
    if (!p || (flags & ~HBS_MP4_HEV1) || !nal || !nal_bytes || n == 0 || n > 65535u || (cap && !out)) return HBS_E_ARG;
    if (p->track_id == 0 || p->track_id == 0xFFFFFFFFu || p->timescale == 0) return HBS_E_ARG;
    if (p->width < 1 || p->width > 65535u || p->height < 1 || p->height > 65535u) return HBS_E_ARG;
    if (p->length_size != 1 && p->length_size != 2 && p->length_size != 4) return HBS_E_ARG;
    if (p->chroma_format_idc < 0 || p->chroma_format_idc > 3) return HBS_E_ARG;
    /* (bitDepthLumaMinus8 / bitDepthChromaMinus8 are three bits in an hvcC) */
    if (p->bit_depth_luma < 8 || p->bit_depth_luma > 15 || p->bit_depth_chroma < 8 || p->bit_depth_chroma > 15) return HBS_E_ARG;
    uint32_t count[3] = {0, 0, 0};
    const uint8_t* sps = nullptr;
    uint64_t sps_bytes = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (!nal[i] || nal_bytes[i] < 2 || nal_bytes[i] > 65535u) return HBS_E_ARG;
        const uint32_t type = (nal[i][0] >> 1) & 0x3Fu;
        if (type < 32 || type > 34) return HBS_E_ARG;
        count[type - 32] += 1;
        if (type == 33 && !sps) { sps = nal[i]; sps_bytes = nal_bytes[i]; }
    }
    uint8_t pre[15];
    if (!sps || mp4_strip_prefix(sps, sps_bytes, pre, 15) < 15) return HBS_E_ARG;
    const bool hev1 = (flags & HBS_MP4_HEV1) != 0;

    for (int pass = 0; pass < 2; ++pass) {
        Mp4Writer w{pass ? out : nullptr, 0};
        const uint64_t ftyp = w.box(HBS_MP4_FOURCC('f', 't', 'y', 'p'));
        w.u32(HBS_MP4_FOURCC('i', 's', 'o', '6')); w.u32(0); w.u32(HBS_MP4_FOURCC('i', 's', 'o', '6')); w.u32(HBS_MP4_FOURCC('m', 'p', '4', '1'));
        w.end(ftyp);
        const uint64_t moov = w.box(HBS_MP4_FOURCC('m', 'o', 'o', 'v'));
        {
            const uint64_t mvhd = w.full(HBS_MP4_FOURCC('m', 'v', 'h', 'd'), 0);
            w.u32(0); w.u32(0); w.u32(p->timescale); w.u32(dur);
            w.u32(0x00010000u); w.u16(0x0100u); w.zeros(10);
            w.matrix(); w.zeros(24); w.u32(p->track_id + 1u);
            w.end(mvhd);
            const uint64_t trak = w.box(HBS_MP4_FOURCC('t', 'r', 'a', 'k'));
            {
                const uint64_t tkhd = w.full(HBS_MP4_FOURCC('t', 'k', 'h', 'd'), 3);
                w.u32(0); w.u32(0); w.u32(p->track_id); w.u32(0); w.u32(dur);
                w.zeros(8); w.u16(0); w.u16(0); w.u16(0); w.u16(0);
                w.matrix(); w.u32(p->width << 16); w.u32(p->height << 16);
                w.end(tkhd);
                const uint64_t mdia = w.box(HBS_MP4_FOURCC('m', 'd', 'i', 'a'));
                {
                    const uint64_t mdhd = w.full(HBS_MP4_FOURCC('m', 'd', 'h', 'd'), 0);
                    w.u32(0); w.u32(0); w.u32(p->timescale); w.u32(dur); w.u16(0x55C4u); w.u16(0);
                    w.end(mdhd);
                    const uint64_t hdlr = w.full(HBS_MP4_FOURCC('h', 'd', 'l', 'r'), 0);
                    w.u32(0); w.u32(HBS_MP4_FOURCC('v', 'i', 'd', 'e')); w.zeros(12);
                    w.bytes(reinterpret_cast<const uint8_t*>("VideoHandler"), 13);
                    w.end(hdlr);
                    const uint64_t minf = w.box(HBS_MP4_FOURCC('m', 'i', 'n', 'f'));
                    {
                        const uint64_t vmhd = w.full(HBS_MP4_FOURCC('v', 'm', 'h', 'd'), 1);
                        w.zeros(8);
                        w.end(vmhd);
                        const uint64_t dinf = w.box(HBS_MP4_FOURCC('d', 'i', 'n', 'f'));
                        const uint64_t dref = w.full(HBS_MP4_FOURCC('d', 'r', 'e', 'f'), 0);
                        w.u32(1);
                        const uint64_t url = w.full(HBS_MP4_FOURCC('u', 'r', 'l', ' '), 1);
                        w.end(url); w.end(dref); w.end(dinf);
                        const uint64_t stbl = w.box(HBS_MP4_FOURCC('s', 't', 'b', 'l'));
                        {
                            const uint64_t stsd = w.full(HBS_MP4_FOURCC('s', 't', 's', 'd'), 0);
                            w.u32(1);
                            const uint64_t entry = w.box(hev1 ? HBS_MP4_FOURCC('h', 'e', 'v', '1') : HBS_MP4_FOURCC('h', 'v', 'c', '1'));
                            w.zeros(6); w.u16(1);
                            w.zeros(16); w.u16(p->width); w.u16(p->height); w.u32(0x00480000u); w.u32(0x00480000u); w.u32(0);
                            w.u16(1); w.zeros(32); w.u16(0x0018u); w.u16(0xFFFFu);
                            const uint64_t hvcc = w.box(HBS_MP4_FOURCC('h', 'v', 'c', 'C'));
                            w.u8(1); w.bytes(pre + 3, 12);
                            w.u8(0xF0); w.u8(0x00); w.u8(0xFC);
                            w.u8(0xFCu | (uint32_t)p->chroma_format_idc);
                            w.u8(0xF8u | (uint32_t)(p->bit_depth_luma - 8)); w.u8(0xF8u | (uint32_t)(p->bit_depth_chroma - 8));
                            w.u16(0);
                            w.u8(((((uint32_t)pre[2] >> 1) & 7u) + 1u) << 3 | ((uint32_t)pre[2] & 1u) << 2 | (uint32_t)(p->length_size - 1));
                            w.u8((count[0] ? 1u : 0u) + (count[1] ? 1u : 0u) + (count[2] ? 1u : 0u));
                            for (uint32_t t = 0; t < 3; ++t) {
                                if (!count[t]) continue;
                                w.u8((hev1 ? 0u : 0x80u) | (32u + t)); w.u16(count[t]);
                                for (uint64_t i = 0; i < n; ++i) {
                                    if ((((uint32_t)nal[i][0] >> 1) & 0x3Fu) != 32u + t) continue;
                                    w.u16((uint32_t)nal_bytes[i]); w.bytes(nal[i], nal_bytes[i]);
                                }
                            }
                            w.end(hvcc); w.end(entry); w.end(stsd);
                            if (!prog) {
                                const uint64_t stts = w.full(HBS_MP4_FOURCC('s', 't', 't', 's'), 0); w.u32(0); w.end(stts);
                                const uint64_t stsc = w.full(HBS_MP4_FOURCC('s', 't', 's', 'c'), 0); w.u32(0); w.end(stsc);
                                const uint64_t stsz = w.full(HBS_MP4_FOURCC('s', 't', 's', 'z'), 0); w.u32(0); w.u32(0); w.end(stsz);
                                const uint64_t stco = w.full(HBS_MP4_FOURCC('s', 't', 'c', 'o'), 0); w.u32(0); w.end(stco);
                            }
                        }
                        w.end(stbl, tb);
                    }
                    w.end(minf, tb);
                }
                w.end(mdia, tb);
            }
            w.end(trak, tb);
            if (!prog) {
                const uint64_t mvex = w.box(HBS_MP4_FOURCC('m', 'v', 'e', 'x'));
                const uint64_t trex = w.full(HBS_MP4_FOURCC('t', 'r', 'e', 'x'), 0);
                w.u32(p->track_id); w.u32(1); w.u32(0); w.u32(0); w.u32(0);
                w.end(trex); w.end(mvex);
            }
        }
        w.end(moov, tb);
        if (prog && w.n - moov + tb > 0xFFFFFFFFull) return HBS_E_ARG;   /* the moov's size has 32 bits */
        if (pass || w.n > cap) return (int64_t)w.n;          /* (the sets are at most 65535 x 65537 bytes: no wrap) */
    }
    return HBS_E_ARG;                                          /* not reached */
}

inline int64_t mp4_init_host(const hbs_mp4_init_params* p, int flags, const uint8_t* const* nal, const uint64_t* nal_bytes, uint64_t n,
                             uint8_t* out, uint64_t cap)
{
    return mp4_moov_build(p, flags, nal, nal_bytes, n, nullptr, out, cap);
}

/* hbs_mp4_moov_host: ftyp and the moov up to and including the stsd; the tables_bytes of hbs_mp4_stbl_write complete it */
inline int64_t mp4_moov_host(const hbs_mp4_init_params* p, int flags, const uint8_t* const* nal, const uint64_t* nal_bytes, uint64_t n,
                             uint64_t duration, uint64_t tables_bytes, uint8_t* out, uint64_t cap)
{
    const Mp4Prog prog{duration, tables_bytes};
    return mp4_moov_build(p, flags, nal, nal_bytes, n, &prog, out, cap);
}

#ifdef __HIPCC__
struct Mp4Args {
    const uint8_t* src; uint64_t n;                   /* the Annex-B stream                                           */
    const hbs_nal_entry* index; uint64_t n_nals;
    const uint8_t* keep;                              /* NULL: all                                                    */
    const uint32_t* nal_au; const hbs_access_unit* au; uint64_t n_aus;
    const unsigned long long* dts; const unsigned long long* pts;      /* nullable                                    */
    uint32_t L, flags, track_id, sequence, max_samples, sample_duration;
    uint64_t base_time;
    uint8_t* out; uint64_t out_cap;                   /* out NULL: plan only                                          */
    unsigned long long* sample_off; unsigned long long* sample_size;   /* nullable, both or neither                   */
    hbs_mp4_frag* frag; uint64_t frag_cap;            /* nullable                                                     */
    hbs_summary* summary;
    /* scratch (lay_mp4) */
    unsigned long long* part_n;    /* 8 per NAL block: record bytes, kept NALs, -, 1 + the lowest bad NAL (0: none)              */
    unsigned long long* part_a;    /* 8 per AU block: fragments that begin in it, 1 + the lowest AU whose fragment is too large  */
    unsigned long long* last;      /* per AU block: 1 + its last AU that s() may name (0: none); then the maximum in front       */
    unsigned long long* bad_a;     /* per AU block: 1 + its lowest AU that breaks a time rule (0: none)                          */
    unsigned long long* ctl;       /* 8: error, output bytes, kept NALs, fragments, bad NAL, bad AU (times), record bytes        */
    unsigned long long* au_B;      /* n_aus + 1: B(a)                                                                            */
    unsigned long long* rec_B;     /* kept + 1: the record bytes in front of kept NAL j (then the total)                         */
    unsigned long long* rec_delta; /* kept: source offset of its payload minus the record offset of its payload                  */
    uint32_t* au_frag;             /* n_aus: the fragment of AU a                                                                */
    unsigned long long* frag_off;  /* R + 1: O_r (then the total)                                                                */
    uint32_t* frag_first;          /* R + 1: f_r (then n_aus)                                                                    */
    unsigned long long* tile_frag; /* tiles + 1: the fragment the output tile's first byte lies in                               */
    unsigned long long* tile_rec;  /* tiles + 1: the kept NAL whose record holds or precedes it                                  */
    uint64_t tiles;                /* output tiles the copy's grid covers                                                        */
    hipEvent_t ev_begin, ev_end;
};

/* the most bytes a call can make: every NAL kept, a fragment a sample */
inline uint64_t mp4_output_bound(uint64_t n_nals, uint64_t n_aus, uint64_t stream_bytes, uint32_t L)
{
    return stream_bytes + n_nals * (uint64_t)L + (16u + kMp4FragFixed) * n_aus;
}
inline uint64_t mp4_tiles(uint64_t reach)
{
    return reach / kMp4TileBytes + (reach % kMp4TileBytes ? 1 : 0);                  /* (reach <= kOutCapMax: below 2^30) */
}

/* scratch: 16 bytes a NAL and 24 an AU of tables with an output (8 an AU without), 64 bytes a plan workgroup of 256 NALs,
 * 80 a plan workgroup of 256 AUs, 16 a 64 KiB output tile */
inline void lay_mp4(Carver& w, Mp4Args& a)
{
    const uint64_t nb = (a.n_nals + kMp4NalsPerBlock - 1) / kMp4NalsPerBlock, ab = (a.n_aus + kMp4AusPerBlock - 1) / kMp4AusPerBlock;
    a.part_n = w.take<unsigned long long>(nb * 64);
    a.part_a = w.take<unsigned long long>(ab * 64);
    a.last = w.take<unsigned long long>(ab * 8);
    a.bad_a = w.take<unsigned long long>(ab * 8);
    a.ctl = w.take<unsigned long long>(64);
    a.au_B = w.take<unsigned long long>((a.n_aus + 1) * 8);
    const bool o = a.out != nullptr;
    a.rec_B = w.take<unsigned long long>(o ? (a.n_nals + 1) * 8 : 0);
    a.rec_delta = w.take<unsigned long long>(o ? a.n_nals * 8 : 0);
    a.au_frag = w.take<uint32_t>(o ? a.n_aus * 4 : 0);
    a.frag_off = w.take<unsigned long long>(o ? (a.n_aus + 1) * 8 : 0);
    a.frag_first = w.take<uint32_t>(o ? (a.n_aus + 1) * 4 : 0);
    a.tile_frag = w.take<unsigned long long>(o ? (a.tiles + 1) * 8 : 0);
    a.tile_rec = w.take<unsigned long long>(o ? (a.tiles + 1) * 8 : 0);
}
hipError_t launch_mp4_fragment(const Mp4Args& a, hipStream_t st);
#endif

} // namespace hbs
#endif
