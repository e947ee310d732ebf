/*
 * hbs_mp4senc.h -- hbs_mp4_senc_samples and hbs_mp4_init_unprotect_host (include/hevcbitstream_amd.h): the rules that read the
 * sample auxiliary information of protected fMP4 fragments back (ISO/IEC 23001-7 senc; 14496-12 saiz as a hint), as host/device
 * inline functions -- mp4senc_find is what one lane does for a fragment (the traf as mp4rd_moof chooses it, its senc, its saiz),
 * mp4senc_header the senc's header, mp4senc_record one sample's record in the serial walk, mp4senc_hint_ok the check of a
 * position that saiz proposes, mp4senc_entry / mp4senc_clear_* / mp4senc_flat_* the entries (the numbering rule is
 * mp4prot_numbering_ok of hbs_mp4prot.h); the kernels of hbs_mp4senc.hip, the host loop below (mp4_senc_samples_host: what tests
 * single-step) and the tests all run them -- the init segment's un-protector (mp4_init_unprotect: plain host code, no GPU; its
 * walk is hbs_mp4box.h's with mp4senc_entry_ok as the test of a stsd entry, and the reader of hbs_mp4rd.h judges what it
 * rebuilt), and the host-visible launcher.  Everything above the launcher compiles with plain g++.
 */
#ifndef HBS_MP4SENC_H
#define HBS_MP4SENC_H

#include <vector>
#include "hbs_mp4prot.h"
#include "hbs_cenc.h"

namespace hbs {

constexpr int kSencLanes = 256;                      /* a fragment, a sample or an entry a lane                               */
constexpr uint64_t kSencEntBlocksMax = 2048;         /* the entry kernel's grid: at most this many workgroups, which stride    */
constexpr uint64_t kSencSubLimit = 1ull << 48;       /* a total of entries at or above this: HBS_E_CAPACITY                    */
constexpr uint64_t kSencFlat = 1ull << 63;           /* rec_at word: a senc without subsamples, the sample is one entry         */
constexpr uint64_t kSencAbsent = 1ull << 62;         /* rec_at word: no senc, the sample is wholly clear                       */
constexpr uint64_t kSencAtMask = kSencAbsent - 1u;   /* (in_bytes is 2^62 at most)                                            */

enum : uint32_t { kSencNone = 0, kSencSub = 1, kSencFlatMode = 2, kSencAbsentMode = 3 };   /* SencFind.mode */
enum : uint32_t { kSencNoHint = 0, kSencHintDefault = 1, kSencHintTable = 2 };             /* SencFind.hint */

/* What the find lane leaves of a fragment: 40 bytes. */
struct SencFind {
    uint64_t data;                 /* where the first sample's record begins: behind version / flags and sample_count         */
    uint64_t end;                  /* the senc box's end                                                                      */
    uint64_t saiz_at;              /* kSencHintTable: where the saiz's size bytes begin                                       */
    uint32_t mode, hint;
    uint32_t def;                  /* kSencHintDefault: default_sample_info_size                                              */
    uint32_t pad;
};

HBS_HD bool mp4_senc_params_ok(const hbs_mp4_senc_params* p)
{
    if (!p || !mp4prot_iv_size_ok(p->iv_size) || (p->flags & ~HBS_SENC_CLEAR_IF_ABSENT) != 0u) return false;
    for (int i = 0; i < 5; ++i) if (p->reserved[i] != 0u) return false;
    return true;
}

/* ---- the rule ------------------------------------------------------------------------------------------------------------ */

/* the senc whose payload (behind the box header) is p[pay, pay + len), in a traf of S samples: version 0, flags 0 or 2,
 * sample_count S */
HBS_HD bool mp4senc_header(const uint8_t* p, uint64_t pay, uint64_t len, uint32_t S, uint32_t& flags)
{
    if (len < 8) return false;
    const uint32_t vf = rd_be32(p, pay);
    flags = vf & 0xFFFFFFu;
    if ((vf >> 24) != 0u || (flags & ~2u) != 0u) return false;
    return rd_be32(p, pay + 4) == S;
}

/* the saiz with that payload as a HINT: usable only when it lies in its box and counts S samples.  Flag 1: aux_info_type and
 * its parameter, 8 bytes more */
HBS_HD void mp4senc_saiz(const uint8_t* p, uint64_t pay, uint64_t len, uint32_t S, SencFind& o)
{
    o.hint = kSencNoHint;
    if (len < 9) return;
    const uint64_t fixed = 9u + ((rd_be32(p, pay) & 1u) ? 8u : 0u);
    if (len < fixed) return;
    const uint64_t q = pay + fixed - 5u;
    const uint32_t def = p[q];
    if (rd_be32(p, q + 1) != S) return;
    if (def) { o.hint = kSencHintDefault; o.def = def; }
    else if (len - fixed >= S) { o.hint = kSencHintTable; o.saiz_at = q + 5u; }
}

/* FIND, a fragment: f in p[0, n), of a call with these params.  false: a fragment error (but for the numbering, and for what
 * only the serial walk sees).  A fragment of no samples has only its bounds checked.  The traf is the one mp4rd_moof reads:
 * the first whose tfhd carries track_id (0: the first traf), every traf in front of it with a well-formed tfhd; every child of
 * the moof and of the trafs up to the chosen one holds the box rule (mp4rd_box).  Of the chosen traf the first senc and the
 * first saiz count.  have_size: the call has a d_sample_size.  No byte outside the fragment is read. */
HBS_HD bool mp4senc_find(const uint8_t* p, uint64_t n, const hbs_mp4_frag& f, uint32_t track_id, uint32_t V, bool have_size, bool clear_if_absent,
                         SencFind& o)
{
    o.data = 0; o.end = 0; o.saiz_at = 0; o.mode = kSencNone; o.hint = kSencNoHint; o.def = 0; o.pad = 0;
    if (f.out_off > n || f.out_bytes > n - f.out_off) return false;
    if (f.samples == 0) return true;
    Mp4Box m;
    if (!mp4rd_box(p, f.out_off, f.out_off + f.out_bytes, m) || m.type != HBS_MP4_FOURCC('m', 'o', 'o', 'f')) return false;
    const uint64_t mend = f.out_off + m.size;
    bool found = false;
    uint64_t t0 = 0, tend = 0;
    for (uint64_t q = f.out_off + m.head; q < mend;) {
        Mp4Box b;
        if (!mp4rd_box(p, q, mend, b)) return false;
        if (b.type == HBS_MP4_FOURCC('t', 'r', 'a', 'f') && !found) {
            Mp4Tfhd h;
            bool have_tfhd = false;
            for (uint64_t c = q + b.head; c < q + b.size;) {
                Mp4Box k;
                if (!mp4rd_box(p, c, q + b.size, k)) return false;
                if (k.type == HBS_MP4_FOURCC('t', 'f', 'h', 'd') && !have_tfhd) {
                    if (!mp4rd_tfhd(p, c + k.head, k.size - k.head, h)) return false;
                    have_tfhd = true;
                }
                c += k.size;
            }
            if (!have_tfhd) return false;
            if (track_id == 0u || h.track_id == track_id) { found = true; t0 = q + b.head; tend = q + b.size; }
        }
        q += b.size;
    }
    if (!found) return false;
    bool have_senc = false, have_saiz = false;
    uint64_t senc_pay = 0, senc_len = 0, saiz_pay = 0, saiz_len = 0;
    for (uint64_t c = t0; c < tend;) {
        Mp4Box k;
        (void)mp4rd_box(p, c, tend, k);                                /* (it held above) */
        if (k.type == HBS_MP4_FOURCC('s', 'e', 'n', 'c') && !have_senc) { have_senc = true; senc_pay = c + k.head; senc_len = k.size - k.head; }
        else if (k.type == HBS_MP4_FOURCC('s', 'a', 'i', 'z') && !have_saiz) { have_saiz = true; saiz_pay = c + k.head; saiz_len = k.size - k.head; }
        c += k.size;
    }
    if (!have_senc) {
        if (!clear_if_absent || !have_size) return false;
        o.mode = kSencAbsentMode;
        return true;
    }
    uint32_t flags;
    if (!mp4senc_header(p, senc_pay, senc_len, f.samples, flags)) return false;
    o.data = senc_pay + 8u; o.end = senc_pay + senc_len;
    if (flags & 2u) {
        o.mode = kSencSub;
        if (have_saiz) mp4senc_saiz(p, saiz_pay, saiz_len, f.samples, o);
        return true;
    }
    /* no subsample tables: sample i's IV lies at data + V i, and its size becomes its one entry */
    if (!have_size || (uint64_t)V * f.samples > o.end - o.data) return false;
    o.mode = kSencFlatMode;
    return true;
}

/* THE SERIAL WALK's step: the record of one sample at `at` of a senc with subsample tables that ends at `end` (at <= end): IV
 * (V bytes) subsample_count(2), then that many clear(2) protect(4).  n: its entries, next: where the next sample's begins.
 * false: it leaves the box */
HBS_HD bool mp4senc_record(const uint8_t* p, uint64_t at, uint64_t end, uint32_t V, uint32_t& n, uint64_t& next)
{
    const uint64_t room = end - at;
    if (room < V + 2u) return false;
    n = rd_be16(p, at + V);
    const uint64_t bytes = V + 2u + 6ull * n;
    if (bytes > room) return false;
    next = at + bytes;
    return true;
}

/* THE HINT CHECK: saiz says that the sample's record has h bytes and that `before` bytes of records lie in front of it.  True
 * when a record of exactly h bytes begins at data + before and stays in the box.  When it holds for every sample of a
 * fragment then, by induction from sample 0 (before = 0), every position is the serial walk's.  Nothing outside the box is
 * read, whatever the saiz holds. */
HBS_HD bool mp4senc_hint_ok(const uint8_t* p, uint64_t data, uint64_t end, uint32_t V, uint64_t before, uint32_t h, uint32_t& n)
{
    const uint64_t room = end - data;
    n = 0;
    if (h < V + 2u || before > room || h > room - before) return false;
    n = rd_be16(p, data + before + V);
    return V + 2u + 6ull * n == h;
}

/* entry j of the record at rec */
HBS_HD hbs_cenc_subsample mp4senc_entry(const uint8_t* p, uint64_t rec, uint32_t V, uint64_t j)
{
    const uint64_t at = rec + V + 2u + 6u * j;
    hbs_cenc_subsample e;
    e.clear = rd_be32(p, at) >> 16; e.protect = rd_be32(p, at + 2);
    return e;
}

/* a wholly clear sample of z bytes (z < 2^32): the entries of hbs_cenc_subsamples' EMIT(z, 0) */
HBS_HD uint64_t mp4senc_clear_count(uint64_t z) { return z ? cenc_entries(z) : 0u; }
HBS_HD hbs_cenc_subsample mp4senc_clear_entry(uint64_t z, uint64_t j) { return cenc_entry(z, 0, j, cenc_entries(z)); }
/* a sample of a senc without subsample tables: (0, z), none when z == 0 */
HBS_HD uint64_t mp4senc_flat_count(uint64_t z) { return z ? 1u : 0u; }

/* the 16 bytes of d_iv for the IV at p + at, as four words in memory order: V bytes, then zeros */
HBS_HD void mp4senc_iv_words(const uint8_t* p, uint64_t at, uint32_t V, uint32_t w[4])
{
    for (uint32_t i = 0; i < 4u; ++i) w[i] = 4u * i < V ? __builtin_bswap32(rd_be32(p, at + 4u * i)) : 0u;
}

/* ---- the call on host memory: the kernels' plan as one loop (tests single-step it) ------------------------------------------ */

struct SencHostOut {
    int32_t error;
    uint64_t bad_sample, bad_frag, senc_read, protect, hinted;       /* hinted: fragments settled by the hint alone */
    std::vector<uint64_t> sub_first;
    std::vector<hbs_cenc_subsample> sub;
    std::vector<uint8_t> iv;
};

inline void mp4_senc_samples_host(const uint8_t* in, uint64_t n, const hbs_mp4_frag* frag, uint64_t R, const uint64_t* size, uint64_t N,
                                  const hbs_mp4_senc_params& prm, SencHostOut& o)
{
    const uint32_t V = prm.iv_size;
    o.error = 0; o.bad_sample = 0; o.bad_frag = 0; o.senc_read = 0; o.protect = 0; o.hinted = 0;
    o.sub_first.assign(N + 1, 0); o.sub.clear(); o.iv.assign(16 * N, 0);
    std::vector<SencFind> find(R);
    std::vector<uint64_t> first(R + 1, 0);
    uint64_t below = 0, stop = 0;                        /* stop: 1 + the lowest fragment that find or the numbering refuses */
    for (uint64_t r = 0; r < R; ++r) {
        const bool ok = mp4senc_find(in, n, frag[r], prm.track_id, V, size != nullptr, (prm.flags & HBS_SENC_CLEAR_IF_ABSENT) != 0u, find[r]);
        if ((!ok || !mp4prot_numbering_ok(frag[r].first_au - frag[0].first_au, below, frag[r].samples, N, r + 1 == R)) && !stop) stop = r + 1;
        first[r] = below;
        below += frag[r].samples;
    }
    std::vector<uint64_t> rec(N, 0), cnt(N, 0);
    /* behind a refused fragment the first samples may mean nothing: the fragments below it are only walked, nothing is kept */
    for (uint64_t r = 0; r < R && !o.bad_frag && (!stop || r + 1 < stop); ++r) {
        const SencFind& f = find[r];
        const uint64_t S = frag[r].samples, s0 = stop ? 0 : first[r];
        if (f.mode == kSencSub || f.mode == kSencFlatMode) o.senc_read += 1;
        if (f.mode == kSencSub) {
            bool all = !stop && f.hint != kSencNoHint;
            uint64_t before = 0;
            for (uint64_t i = 0; i < S && all; ++i) {                  /* count, hinted */
                const uint32_t h = f.hint == kSencHintDefault ? f.def : in[f.saiz_at + i];
                uint32_t c;
                all = mp4senc_hint_ok(in, f.data, f.end, V, before, h, c);
                rec[s0 + i] = f.data + before; cnt[s0 + i] = c;
                before += h;
            }
            if (all) { o.hinted += 1; continue; }
            uint64_t at = f.data;
            for (uint64_t i = 0; i < S; ++i) {                         /* count, serial */
                uint32_t c;
                uint64_t next;
                if (!mp4senc_record(in, at, f.end, V, c, next)) { o.bad_frag = r + 1; break; }
                if (!stop) { rec[s0 + i] = at; cnt[s0 + i] = c; }
                at = next;
            }
        } else if (f.mode != kSencNone && !stop) {
            for (uint64_t i = 0; i < S; ++i) {
                const uint64_t z = size[s0 + i];
                if (z > 0xFFFFFFFFull) { if (!o.bad_sample) o.bad_sample = s0 + i + 1; continue; }
                rec[s0 + i] = f.mode == kSencFlatMode ? (f.data + (uint64_t)V * i) | kSencFlat : kSencAbsent;
                cnt[s0 + i] = f.mode == kSencFlatMode ? mp4senc_flat_count(z) : mp4senc_clear_count(z);
            }
        }
    }
    if (!o.bad_frag) o.bad_frag = stop;
    if (o.bad_frag) { o.bad_sample = 0; o.senc_read = 0; o.error = HBS_E_ARG; return; }
    if (o.bad_sample) { o.senc_read = 0; o.error = HBS_E_ARG; return; }
    for (uint64_t s = 0; s < N; ++s) {
        o.sub_first[s + 1] = o.sub_first[s] + cnt[s];
        for (uint64_t j = 0; j < cnt[s]; ++j) {
            hbs_cenc_subsample e;
            if (rec[s] & kSencFlat) { e.clear = 0; e.protect = (uint32_t)size[s]; }
            else if (rec[s] & kSencAbsent) e = mp4senc_clear_entry(size[s], j);
            else e = mp4senc_entry(in, rec[s], V, j);
            o.protect += e.protect;
            o.sub.push_back(e);
        }
        if (V && !(rec[s] & kSencAbsent)) {
            uint32_t w[4];
            mp4senc_iv_words(in, rec[s] & kSencAtMask, V, w);
            memcpy(o.iv.data() + 16 * s, w, 16);
        }
    }
}

/* ---- the init segment ---------------------------------------------------------------------------------------------------- */

struct SencEntry { uint64_t sinf_at, sinf_bytes; uint32_t format; hbs_mp4_tenc t; };

/* the sinf whose children are p[at, end): frma in {hvc1, hev1}, schm cenc or cbcs, schi / tenc of version 0 or 1 with
 * isProtected 1 and an IV rule that hbs_mp4_tenc can state */
inline bool mp4senc_sinf(const uint8_t* p, uint64_t at, uint64_t end, SencEntry& e)
{
    Mp4At b, schi;
    memset(&e.t, 0, sizeof(e.t));
    if (mp4_child(p, at, end, HBS_MP4_FOURCC('f', 'r', 'm', 'a'), b) <= 0 || b.size - b.head < 4) return false;
    e.format = rd_be32(p, b.pay());
    if (e.format != HBS_MP4_FOURCC('h', 'v', 'c', '1') && e.format != HBS_MP4_FOURCC('h', 'e', 'v', '1')) return false;
    if (mp4_child(p, at, end, HBS_MP4_FOURCC('s', 'c', 'h', 'm'), b) <= 0 || b.size - b.head < 8) return false;
    e.t.scheme = rd_be32(p, b.pay() + 4);
    if (mp4_child(p, at, end, HBS_MP4_FOURCC('s', 'c', 'h', 'i'), schi) <= 0) return false;
    if (mp4_child(p, schi.pay(), schi.end(), HBS_MP4_FOURCC('t', 'e', 'n', 'c'), b) <= 0 || b.size - b.head < 24) return false;
    const uint64_t a = b.pay(), z = b.end();
    const uint32_t version = p[a];
    if (version > 1u || p[a + 6] != 1u) return false;
    if (version == 1u) { e.t.crypt_byte_block = p[a + 5] >> 4; e.t.skip_byte_block = p[a + 5] & 15u; }
    e.t.iv_size = p[a + 7];
    memcpy(e.t.kid, p + a + 8, 16);
    if (e.t.iv_size == 0u) {
        if (z - a < 25) return false;
        e.t.constant_iv_size = p[a + 24];
        if ((e.t.constant_iv_size != 8u && e.t.constant_iv_size != 16u) || z - a < 25u + e.t.constant_iv_size) return false;
        memcpy(e.t.constant_iv, p + a + 25, e.t.constant_iv_size);
    }
    return mp4_tenc_ok(&e.t);
}

/* the test of a stsd entry: a resizable 'encv' that holds an hvcC and a sinf that mp4senc_sinf accepts (se: what it said) */
inline bool mp4senc_entry_ok(const uint8_t* p, uint32_t type, const Mp4At& e, SencEntry& se)
{
    if (type != HBS_MP4_FOURCC('e', 'n', 'c', 'v') || !mp4_resizable(p, e) || e.size - e.head < 78) return false;
    const uint64_t ca = e.pay() + 78u, ce = e.end();
    Mp4At h, s;
    if (mp4_child(p, ca, ce, HBS_MP4_FOURCC('h', 'v', 'c', 'C'), h) <= 0 || mp4_child(p, ca, ce, HBS_MP4_FOURCC('s', 'i', 'n', 'f'), s) <= 0) return false;
    if (!mp4senc_sinf(p, s.pay(), s.end(), se)) return false;
    se.sinf_at = s.pos; se.sinf_bytes = s.size;
    return true;
}

/* k.box[kPathTrak] is a protected video track whose boxes can shrink in place (k: its path); nothing behind them is looked at */
inline bool mp4senc_track(const uint8_t* p, Mp4TrackPath& k, SencEntry& entry)
{
    const auto test = [&](uint32_t type, const Mp4At& e) -> int { return mp4senc_entry_ok(p, type, e, entry) ? 1 : 0; };
    if (mp4_track_descend(p, k, false, test) <= 0) return false;
    for (int i = kPathMdia; i <= kPathStsd; ++i) if (!mp4_resizable(p, k.box[i])) return false;
    return true;
}

/* hbs_mp4_init_unprotect_host */
inline int64_t mp4_init_unprotect(const uint8_t* init, uint64_t n, uint32_t track_id, hbs_mp4_tenc* t_out, uint32_t* format_out,
                                  uint64_t* pssh_off, uint64_t* pssh_bytes, uint64_t pssh_cap, uint64_t* n_pssh_out, uint8_t* out, uint64_t cap)
{
    if (!init || !t_out || n > kRdMaxIn || (cap && !out) || (pssh_cap && (!pssh_off || !pssh_bytes))) return HBS_E_ARG;
    /* 1. the moov's children: the pssh boxes leave, and each trak with a 32-bit size is tried until one is found */
    Mp4TrackPath path, k;
    if (mp4_child(init, 0, n, HBS_MP4_FOURCC('m', 'o', 'o', 'v'), k.box[kPathMoov]) <= 0 || !mp4_resizable(init, k.box[kPathMoov])) return HBS_E_ARG;
    const Mp4At moov = k.box[kPathMoov];
    struct Cut { uint64_t at, bytes; };
    std::vector<Cut> cuts;                               /* what leaves the segment, in the order it lies there */
    uint64_t n_pssh = 0, pssh_total = 0;
    bool found = false;
    uint32_t found_id = 0;
    SencEntry entry;
    for (uint64_t at = moov.pay(); at < moov.end();) {
        Mp4Box b;
        if (!mp4rd_box(init, at, moov.end(), b)) return HBS_E_ARG;
        k.box[kPathTrak] = Mp4At{at, b.size, b.head};
        if (b.type == HBS_MP4_FOURCC('p', 's', 's', 'h')) {
            cuts.push_back(Cut{at, b.size});
            pssh_total += b.size; n_pssh += 1;
        } else if (b.type == HBS_MP4_FOURCC('t', 'r', 'a', 'k') && !found && mp4_resizable(init, k.box[kPathTrak])) {
            Mp4Tkhd h;
            if (!mp4_tkhd(init, at + b.head, at + b.size, h)) return HBS_E_ARG;
            if ((track_id == 0u || h.track_id == track_id) && mp4senc_track(init, k, entry)) {
                found = true; found_id = h.track_id; path = k;
                cuts.push_back(Cut{entry.sinf_at, entry.sinf_bytes});
            }
        }
        at += b.size;
    }
    if (!found) return HBS_E_ARG;
    /* 2. the clear segment, made whole: the cuts closed, the seven sizes reduced, the entry named as the frma says */
    const uint64_t need = n - entry.sinf_bytes - pssh_total;
    std::vector<uint8_t> seg;
    seg.reserve(need);
    uint64_t from = 0;
    for (const Cut& c : cuts) { seg.insert(seg.end(), init + from, init + c.at); from = c.at + c.bytes; }
    seg.insert(seg.end(), init + from, init + n);
    for (int i = 0; i < kPathBoxes; ++i) {
        uint64_t shift = 0;                              /* what was cut in front of the box */
        for (const Cut& c : cuts) if (c.at < path.box[i].pos) shift += c.bytes;
        uint8_t* q = seg.data() + (path.box[i].pos - shift);
        wr_be32(q, (uint32_t)path.box[i].size - (uint32_t)entry.sinf_bytes - (i == kPathMoov ? (uint32_t)pssh_total : 0u));
        if (i == kPathEntry) wr_be32(q + 4, entry.format);
    }
    /* 3. the reader's verdict on it */
    hbs_mp4_track trk;
    if (mp4_init_read_host(seg.data(), need, found_id, &trk, nullptr, nullptr, 0) < 0 || trk.entry != entry.format) return HBS_E_ARG;
    *t_out = entry.t;
    if (format_out) *format_out = entry.format;
    if (n_pssh_out) *n_pssh_out = n_pssh;
    uint64_t j = 0;
    for (const Cut& c : cuts) {
        if (c.at == entry.sinf_at) continue;
        if (j < pssh_cap) { pssh_off[j] = c.at; pssh_bytes[j] = c.bytes; }
        j += 1;
    }
    if (need <= cap) memcpy(out, seg.data(), need);
    return (int64_t)need;
}

#ifdef __HIPCC__
struct Mp4SencArgs {
    const uint8_t* src; uint64_t n;                   /* d_in                                                          */
    const hbs_mp4_frag* frag; uint64_t n_frags;
    const unsigned long long* sample_size; uint64_t n_samples;        /* sample_size nullable                          */
    uint32_t V, track_id, flags;
    unsigned long long* sub_first; hbs_cenc_subsample* sub; uint64_t sub_cap;   /* sub NULL: plan only                 */
    uint8_t* iv;
    hbs_summary* summary;
    /* scratch (lay_mp4senc) */
    unsigned long long* part_f;    /* 8 per fragment block: samples, fragments with a senc; 1 + the lowest fragment find refuses   */
    unsigned long long* bad_num;   /* per fragment block: 1 + its lowest fragment that breaks the numbering rule (0: none)          */
    unsigned long long* bad_walk;  /* per fragment block: 1 + its lowest fragment whose senc a sample leaves                        */
    unsigned long long* part_k;    /* 8 per sample block: the open sum of the hint's sizes of its last fragment, whether one began  */
    unsigned long long* part_c;    /* 8 per sample block: entries; 1 + its lowest sample whose size cannot be an entry              */
    unsigned long long* part_p;    /* 8 per entry block: the sum of protect                                                         */
    unsigned long long* ctl;       /* 8: kSenc* below                                                                               */
    SencFind* find;                /* R                                                                                             */
    unsigned long long* frag_first;/* R + 1: the fragment's first sample (then n_samples)                                           */
    uint32_t* frag_fail;           /* R: a sample's hint check failed: the fragment is walked                                       */
    unsigned long long* rec_at;    /* N: where the sample's record lies | kSencFlat | kSencAbsent                                   */
    unsigned long long* first;     /* N + 1: the sample's entries, then the entries in front of it                                  */
    uint64_t ent_blocks;           /* the entry kernel's grid                                                                       */
    hipEvent_t ev_begin, ev_end;
};

/* scratch: 64 bytes; 52 bytes a fragment and 80 per 256 of them; 16 bytes a sample, 128 per 256 of them and 64 per entry
 * workgroup, of which there are min(2 048, 4 per 256 samples); every table rounded up to 256 bytes */
inline void lay_mp4senc(Carver& w, Mp4SencArgs& a)
{
    const uint64_t fb = (a.n_frags + kSencLanes - 1) / kSencLanes, sb = (a.n_samples + kSencLanes - 1) / kSencLanes;
    a.ent_blocks = 4 * sb < kSencEntBlocksMax ? 4 * sb : kSencEntBlocksMax;
    a.part_f = w.take<unsigned long long>(fb * 64);
    a.bad_num = w.take<unsigned long long>(fb * 8);
    a.bad_walk = w.take<unsigned long long>(fb * 8);
    a.part_k = w.take<unsigned long long>(sb * 64);
    a.part_c = w.take<unsigned long long>(sb * 64);
    a.part_p = w.take<unsigned long long>(a.ent_blocks * 64);
    a.ctl = w.take<unsigned long long>(64);
    a.find = w.take<SencFind>(a.n_frags * sizeof(SencFind));
    a.frag_first = w.take<unsigned long long>((a.n_frags + 1) * 8);
    a.frag_fail = w.take<uint32_t>(a.n_frags * 4);
    a.rec_at = w.take<unsigned long long>(a.n_samples * 8);
    a.first = w.take<unsigned long long>((a.n_samples + 1) * 8);
}
hipError_t launch_mp4_senc_samples(const Mp4SencArgs& a, hipStream_t st);
#endif

} // namespace hbs
#endif
