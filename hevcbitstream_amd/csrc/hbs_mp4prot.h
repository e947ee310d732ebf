/*
 * hbs_mp4prot.h -- hbs_mp4_protect and hbs_mp4_init_protect_host (include/hevcbitstream_amd.h): the rule that turns one fMP4
 * fragment of hbs_mp4_fragment into a protected one (saiz, saio and senc behind the trun; ISO/IEC 14496-12 and 23001-7), as
 * host/device inline functions -- mp4prot_frag_ok is the fragment rule, mp4prot_sample_tables and mp4prot_sample_entries the two
 * groups of the sample rule, mp4prot_moof_byte the byte at a moof-relative offset of the output; the kernels of
 * hbs_mp4prot.hip, the host checks and the tests all run them -- the init segment's rewriter (mp4_init_protect: plain host code,
 * no GPU; it grows the seven boxes of the reader's Mp4TrackPath), and the host-visible launcher.  Above that: plain g++.
 */
#ifndef HBS_MP4PROT_H
#define HBS_MP4PROT_H

#include "hbs_mp4rd.h"

namespace hbs {

constexpr int kProtLanes = 256;                      /* plan: a fragment or a sample a lane                           */
constexpr uint64_t kProtTileBytes = 64 * 1024;       /* copy: output bytes of one workgroup                           */
constexpr uint32_t kProtFixed = 53;                  /* what a fragment grows by besides (V + 3) S + 6 E              */
constexpr uint32_t kProtMoofFixed = 141;             /* the new moof's bytes besides (19 + V) S + 6 E                 */
constexpr uint64_t kProtMoofMax = 0x7FFFFFFFull - 8u;/* the trun's data_offset, moof + 8, is a signed 32-bit field    */
constexpr uint64_t kProtSubLimit = 1ull << 48;       /* a d_sub_first word at or above this is an error (hbs_cenc_crypt's limit) */
constexpr uint64_t kProtBytesLimit = 1ull << 41;     /* sum of floor(out_bytes / 2^20) + n_frags at or above this: the output
                                                        could pass 2^61, HBS_E_CAPACITY                                 */

HBS_HD uint64_t mp4prot_growth(uint64_t S, uint64_t E, uint32_t V) { return kProtFixed + (V + 3ull) * S + 6u * E; }
HBS_HD uint64_t mp4prot_moof_bytes(uint64_t S, uint64_t E, uint32_t V) { return kProtMoofFixed + (19ull + V) * S + 6u * E; }
HBS_HD uint32_t mp4prot_max_entries(uint32_t V) { return (253u - V) / 6u; }      /* the saiz byte V + 2 + 6 n fits */
HBS_HD bool mp4prot_iv_size_ok(uint32_t V) { return V == 0u || V == 8u || V == 16u; }

/* ---- the fragment rule --------------------------------------------------------------------------------------------------- */

/* THE FRAGMENT RULE but for the numbering: f is, in in[0, in_bytes), a fragment in the form hbs_mp4_fragment states.  The
 * words that are looked at are those mp4_head_word gives for f, less the mfhd, the tfhd's and the tfdt's own (sequence, track
 * id and decode time are not constrained).  Reads no byte outside the fragment, and none when its range is wrong. */
HBS_HD bool mp4prot_frag_ok(const uint8_t* in, uint64_t in_bytes, const hbs_mp4_frag& f)
{
    if (f.out_off > in_bytes || f.out_bytes > in_bytes - f.out_off) return false;
    if (f.samples > kMp4MaxSamples) return false;
    const uint64_t head = kMp4MoofHead + 16ull * f.samples;
    if (f.out_bytes < head + 8u || f.out_bytes - head > 0xFFFFFFFFull) return false;
    /* moof size and type, traf size and type, the types of tfhd and tfdt, the trun's five words */
    const uint32_t looked_at = 1u << 0 | 1u << 1 | 1u << 6 | 1u << 7 | 1u << 9 | 1u << 13 | 1u << 17 | 1u << 18 | 1u << 19 | 1u << 20 | 1u << 21;
    for (uint32_t w = 0; w < 22u; ++w)
        if ((looked_at >> w & 1u) && rd_be32(in, f.out_off + 4u * w) != mp4_head_word(f, 0, w)) return false;
    return rd_be32(in, f.out_off + head) == mp4_head_word(f, 0, 22) && rd_be32(in, f.out_off + head + 4) == mp4_head_word(f, 0, 23);
}

/* the numbering rule of a fragment of S samples whose first_au lies `rel` behind that of fragment 0, with `below` samples in
 * the fragments below it: its samples are [below, below + S) of the call's n_samples, and the last fragment ends them */
HBS_HD bool mp4prot_numbering_ok(uint64_t rel, uint64_t below, uint64_t S, uint64_t n_samples, bool last)
{
    if (rel != below || below > n_samples || S > n_samples - below) return false;
    return !last || below + S == n_samples;
}

/* ---- the sample rule ----------------------------------------------------------------------------------------------------- */

/* FIRST GROUP, sample s of the call: what the tables say without an entry being read.  sub_first: the call's (n_samples + 1
 * words), iv: the call's (read with V == 8 only) */
HBS_HD bool mp4prot_sample_tables(const uint64_t* sub_first, const uint8_t* iv, uint32_t V, uint64_t s)
{
    const uint64_t a = sub_first[s], b = sub_first[s + 1];
    if ((s == 0 && a != 0) || b < a || b >= kProtSubLimit || b - a > mp4prot_max_entries(V)) return false;
    if (V == 8u)
        for (uint32_t i = 8; i < 16; ++i) if (iv[16u * s + i] != 0) return false;
    return true;
}

/* SECOND GROUP, only when the first holds for every sample: the entries sub[first, first + n) have clear <= 65535 and add up
 * to `size`, the size word of the sample's trun entry */
HBS_HD bool mp4prot_sample_entries(const hbs_cenc_subsample* sub, uint64_t first, uint32_t n, uint32_t size)
{
    uint64_t sum = 0;
    for (uint32_t e = 0; e < n; ++e) {
        const hbs_cenc_subsample x = sub[first + e];
        if (x.clear > 65535u) return false;
        sum += (uint64_t)x.clear + x.protect;
    }
    return sum == size;
}

/* ---- the bytes of the new moof ------------------------------------------------------------------------------------------- */

HBS_HD uint32_t mp4prot_be_byte(uint32_t word, uint64_t at) { return (word >> (8u * (3u - (uint32_t)(at & 3u)))) & 0xFFu; }

/* where the auxiliary data of sample i of a fragment begins in its senc, behind the senc's 16 bytes of header; sf: the
 * fragment's window of d_sub_first (sf[i] belongs to its sample i) */
HBS_HD uint64_t mp4prot_aux_at(const uint64_t* sf, uint32_t V, uint64_t i) { return (V + 2ull) * i + 6u * (sf[i] - sf[0]); }

/* THE RULE: byte m, m < M' = mp4prot_moof_bytes(S, E, V), of the moof of the protected fragment made of the fragment of S
 * samples at in + in_off.  sf and iv: the windows of d_sub_first and d_iv that begin at the fragment's first sample (sf[S] -
 * sf[0] == E; neither is read when S == 0, iv not when V == 0); sub: the call's entries.  Bytes behind the moof are the old
 * fragment's from its mdat header on: output byte m >= M' is in[in_off + 88 + 16 S + (m - M')]. */
HBS_HD uint32_t mp4prot_moof_byte(const uint8_t* in, uint64_t in_off, uint32_t S, uint64_t E, uint32_t V, const uint64_t* sf,
                                  const hbs_cenc_subsample* sub, const uint8_t* iv, uint64_t m)
{
    const uint64_t head = kMp4MoofHead + 16ull * S;
    const uint32_t moof = (uint32_t)mp4prot_moof_bytes(S, E, V);                 /* (at most kProtMoofMax) */
    if (m < head) {                                     /* mfhd, tfhd, tfdt and trun as they are, but for three words */
        const uint64_t w = m >> 2;
        if (w == 0u) return mp4prot_be_byte(moof, m);
        if (w == 6u) return mp4prot_be_byte(moof - 24u, m);
        if (w == 21u) return mp4prot_be_byte(moof + 8u, m);
        return in[in_off + m];
    }
    uint64_t q = m - head;
    if (q < 17ull + S) {                                /* saiz */
        if (q >= 17u) return V + 2u + 6u * (uint32_t)(sf[q - 16u] - sf[q - 17u]);
        if (q >= 13u) return mp4prot_be_byte(S, q - 13u);
        if (q >= 8u) return 0u;
        return mp4prot_be_byte(q < 4u ? 17u + S : HBS_MP4_FOURCC('s', 'a', 'i', 'z'), q);
    }
    q -= 17ull + S;
    if (q < 20u) {                                      /* saio: one offset, from the moof's first byte to the senc's data */
        const uint32_t w = (uint32_t)q >> 2;
        return mp4prot_be_byte(w == 0u ? 20u : w == 1u ? HBS_MP4_FOURCC('s', 'a', 'i', 'o') : w == 2u ? 0u : w == 3u ? 1u : kProtMoofFixed + 17u * S, q);
    }
    q -= 20u;
    if (q < 16u) {                                      /* senc: version 0, flags 2 (subsamples) */
        const uint32_t w = (uint32_t)q >> 2;
        return mp4prot_be_byte(w == 0u ? moof - (kProtMoofFixed - 16u) - 17u * S : w == 1u ? HBS_MP4_FOURCC('s', 'e', 'n', 'c') : w == 2u ? 2u : S, q);
    }
    q -= 16u;
    uint64_t lo = 0, hi = S - 1u;                       /* the last sample whose auxiliary data begins at or in front of q */
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1u) >> 1;
        if (mp4prot_aux_at(sf, V, mid) <= q) lo = mid; else hi = mid - 1u;
    }
    uint64_t j = q - mp4prot_aux_at(sf, V, lo);
    if (j < V) return iv[16u * lo + j];
    j -= V;
    if (j < 2u) return (uint32_t)((sf[lo + 1u] - sf[lo]) >> (8u * (1u - (uint32_t)j))) & 0xFFu;
    j -= 2u;
    const hbs_cenc_subsample x = sub[sf[lo] + j / 6u];
    const uint32_t k = (uint32_t)(j % 6u);
    return k < 2u ? (x.clear >> (8u * (1u - k))) & 0xFFu : (x.protect >> (8u * (5u - k))) & 0xFFu;
}

/* ---- host side ----------------------------------------------------------------------------------------------------------- */

inline bool mp4_protect_params_ok(const hbs_mp4_protect_params* p)
{
    if (!p || !mp4prot_iv_size_ok(p->iv_size) || p->flags != 0u) return false;
    for (int i = 0; i < 6; ++i) if (p->reserved[i] != 0u) return false;
    return true;
}

/* the protected fragment of f (which holds the fragment rule, and whose samples hold the sample rule) into out[0, f.out_bytes +
 * mp4prot_growth(S, E, V)): the moof through the rule, byte by byte, then the mdat; sf, iv: as mp4prot_moof_byte's */
inline void mp4prot_write_fragment_host(const uint8_t* in, const hbs_mp4_frag& f, uint32_t V, const uint64_t* sf, const hbs_cenc_subsample* sub,
                                        const uint8_t* iv, uint8_t* out)
{
    const uint64_t E = f.samples ? sf[f.samples] - sf[0] : 0, moof = mp4prot_moof_bytes(f.samples, E, V);
    for (uint64_t m = 0; m < moof; ++m) out[m] = (uint8_t)mp4prot_moof_byte(in, f.out_off, f.samples, E, V, sf, sub, iv, m);
    const uint64_t head = kMp4MoofHead + 16ull * f.samples;
    for (uint64_t m = head; m < f.out_bytes; ++m) out[moof + (m - head)] = in[f.out_off + m];
}

constexpr uint32_t kTencCenc = HBS_MP4_FOURCC('c', 'e', 'n', 'c'), kTencCbcs = HBS_MP4_FOURCC('c', 'b', 'c', 's');

inline bool mp4_tenc_ok(const hbs_mp4_tenc* t)
{
    if (!t || (t->scheme != kTencCenc && t->scheme != kTencCbcs)) return false;
    if (t->crypt_byte_block > 15u || t->skip_byte_block > 15u) return false;
    if (t->scheme == kTencCenc && (t->crypt_byte_block | t->skip_byte_block) != 0u) return false;
    if (!mp4prot_iv_size_ok(t->iv_size)) return false;
    if (t->iv_size == 0u ? (t->constant_iv_size != 8u && t->constant_iv_size != 16u) : t->constant_iv_size != 0u) return false;
    for (int i = 0; i < 6; ++i) if (t->reserved[i] != 0u) return false;
    return true;
}

/* the sinf of a sample entry that was `fourcc`: frma, schm, schi with the tenc */
inline void mp4prot_sinf(Mp4Writer& w, uint32_t fourcc, const hbs_mp4_tenc& t)
{
    const uint64_t sinf = w.box(HBS_MP4_FOURCC('s', 'i', 'n', 'f'));
    const uint64_t frma = w.box(HBS_MP4_FOURCC('f', 'r', 'm', 'a')); w.u32(fourcc); w.end(frma);
    const uint64_t schm = w.full(HBS_MP4_FOURCC('s', 'c', 'h', 'm'), 0); w.u32(t.scheme); w.u32(0x00010000u); w.end(schm);
    const uint64_t schi = w.box(HBS_MP4_FOURCC('s', 'c', 'h', 'i'));
    const bool pattern = (t.crypt_byte_block | t.skip_byte_block) != 0u;
    const uint64_t tenc = w.box(HBS_MP4_FOURCC('t', 'e', 'n', 'c'));
    w.u32(pattern ? 0x01000000u : 0u);
    w.u8(0); w.u8(pattern ? (uint32_t)t.crypt_byte_block << 4 | t.skip_byte_block : 0u); w.u8(1); w.u8(t.iv_size);
    w.bytes(t.kid, 16);
    if (t.iv_size == 0u) { w.u8(t.constant_iv_size); w.bytes(t.constant_iv, t.constant_iv_size); }
    w.end(tenc); w.end(schi); w.end(sinf);
}

/* hbs_mp4_init_protect_host */
inline int64_t mp4_init_protect(const uint8_t* init, uint64_t n, uint32_t track_id, const hbs_mp4_tenc* t, const uint8_t* const* pssh,
                                const uint64_t* pssh_bytes, uint64_t n_pssh, uint8_t* out, uint64_t cap)
{
    if (!init || n > kRdMaxIn || !mp4_tenc_ok(t) || (n_pssh && (!pssh || !pssh_bytes)) || (cap && !out)) return HBS_E_ARG;
    uint64_t pssh_total = 0;
    for (uint64_t i = 0; i < n_pssh; ++i) {
        const uint64_t k = pssh_bytes[i];
        if (!pssh[i] || k < 8u || k > 0xFFFFFFFFull || rd_be32(pssh[i], 0) != k || rd_be32(pssh[i], 4) != HBS_MP4_FOURCC('p', 's', 's', 'h')) return HBS_E_ARG;
        pssh_total += k;
        if (pssh_total > 0xFFFFFFFFull) return HBS_E_ARG;
    }
    /* the track, by the reader itself, which leaves the boxes that hold the hvcC: moov, trak, mdia, minf, stbl, stsd, the entry */
    hbs_mp4_track trk;
    Mp4TrackPath path;
    if (mp4_init_read_host(init, n, track_id, &trk, nullptr, nullptr, 0, &path) < 0) return HBS_E_ARG;
    Mp4Writer sw{nullptr, 0};
    mp4prot_sinf(sw, 0, *t);
    const uint64_t sinf_bytes = sw.n;
    uint32_t size[kPathBoxes];
    for (int i = 0; i < kPathBoxes; ++i) {
        const Mp4At& b = path.box[i];
        if (!mp4_resizable(init, b)) return HBS_E_ARG;
        const uint64_t grown = b.size + sinf_bytes + (i == kPathMoov ? pssh_total : 0);
        if (grown > 0xFFFFFFFFull) return HBS_E_ARG;
        size[i] = (uint32_t)grown;
    }
    const Mp4At& entry = path.box[kPathEntry];
    const uint64_t entry_end = entry.end(), moov_end = path.box[kPathMoov].end();
    const uint32_t fourcc = rd_be32(init, entry.pos + 4);
    if (fourcc != trk.entry) return HBS_E_ARG;
    const uint64_t need = n + sinf_bytes + pssh_total;
    if (need > cap) return (int64_t)need;
    Mp4Writer w{out, 0};
    w.bytes(init, entry_end);
    mp4prot_sinf(w, fourcc, *t);
    w.bytes(init + entry_end, moov_end - entry_end);
    for (uint64_t i = 0; i < n_pssh; ++i) w.bytes(pssh[i], pssh_bytes[i]);
    w.bytes(init + moov_end, n - moov_end);
    for (int i = 0; i < kPathBoxes; ++i) wr_be32(out + path.box[i].pos, size[i]);
    memcpy(out + entry.pos + 4, "encv", 4);
    return (int64_t)need;
}

#ifdef __HIPCC__
struct Mp4ProtArgs {
    const uint8_t* src; uint64_t n;                   /* d_in                                                          */
    const hbs_mp4_frag* frag; uint64_t n_frags;
    const unsigned long long* sub_first; const hbs_cenc_subsample* sub; const uint8_t* iv; uint64_t n_samples;
    uint32_t V;
    uint8_t* out; uint64_t out_cap;                   /* out NULL: plan only                                           */
    unsigned long long* sample_off; unsigned long long* sample_size;   /* nullable, both or neither                    */
    hbs_mp4_frag* frag_out;                           /* nullable                                                      */
    hbs_summary* summary;
    /* scratch (lay_mp4prot) */
    unsigned long long* part_f;    /* 8 per fragment block: samples, bytes, bytes / 2^20; 1 + the lowest fragment not in the form   */
    unsigned long long* bad_num;   /* per fragment block: 1 + its lowest fragment that breaks the numbering rule (0: none)          */
    unsigned long long* bad_big;   /* per fragment block: 1 + its lowest fragment whose new moof is too large                      */
    unsigned long long* bad_tab;   /* per sample block: 1 + its lowest sample that fails the first group                            */
    unsigned long long* bad_ent;   /* per sample block: ... the second                                                              */
    unsigned long long* part_k;    /* 8 per sample block: the open sum of the sizes of its last fragment's samples, whether one began */
    unsigned long long* ctl;       /* 8: error, output bytes, bad fragment, bad sample (first group), input fragment bytes, too large */
    unsigned long long* frag_first;/* R + 1: the fragment's first sample (then n_samples)                                           */
    unsigned long long* frag_at;   /* R + 1: where it begins in the output (then the total)                                         */
    unsigned long long* frag_body; /* R: where its mdat header begins in the output                                                 */
    unsigned long long* frag_delta;/* R: source offset minus output offset of the bytes from there on                               */
    unsigned long long* tile_frag; /* tiles + 1: the fragment the output tile's first byte lies in                                  */
    uint64_t tiles;                /* output tiles the copy's grid covers                                                           */
    hipEvent_t ev_begin, ev_end;
};

inline uint64_t mp4prot_tiles(uint64_t out_cap)
{
    return out_cap / kProtTileBytes + (out_cap % kProtTileBytes ? 1 : 0);            /* (out_cap <= kOutCapMax: at most 2^30) */
}

/* scratch: 64 bytes and three 256-byte lines, then 32 bytes a fragment and 80 per 256 of them, 80 bytes per 256 samples, and
 * with an output 8 bytes a 64 KiB tile of out_cap; every table rounded up to 256 bytes */
inline void lay_mp4prot(Carver& w, Mp4ProtArgs& a)
{
    const uint64_t fb = (a.n_frags + kProtLanes - 1) / kProtLanes, sb = (a.n_samples + kProtLanes - 1) / kProtLanes;
    a.part_f = w.take<unsigned long long>(fb * 64);
    a.bad_num = w.take<unsigned long long>(fb * 8);
    a.bad_big = w.take<unsigned long long>(fb * 8);
    a.bad_tab = w.take<unsigned long long>(sb * 8);
    a.bad_ent = w.take<unsigned long long>(sb * 8);
    a.part_k = w.take<unsigned long long>(sb * 64);
    a.ctl = w.take<unsigned long long>(64);
    a.frag_first = w.take<unsigned long long>((a.n_frags + 1) * 8);
    a.frag_at = w.take<unsigned long long>((a.n_frags + 1) * 8);
    a.frag_body = w.take<unsigned long long>(a.n_frags * 8);
    a.frag_delta = w.take<unsigned long long>(a.n_frags * 8);
    a.tile_frag = w.take<unsigned long long>(a.out ? (a.tiles + 1) * 8 : 0);
}
hipError_t launch_mp4_protect(const Mp4ProtArgs& a, hipStream_t st);
#endif

} // namespace hbs
#endif
