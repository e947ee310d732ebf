/*
 * hbs_cenc.h -- hbs_cenc_subsamples and hbs_cenc_crypt (include/hevcbitstream_amd.h): the rules as host/device inline functions
 * -- cenc_te0 / cenc_expand_key / cenc_aes_block are AES-128 (FIPS-197) over one table of 256 words, cenc_ctr_* the counter
 * rule of ISO/IEC 23001-7 `cenc` (the addition stays in bytes 8..15), cenc_nal_split / cenc_entries / cenc_entry /
 * cenc_nal_entries the subsample rule, cenc_plan_params_ok / cenc_params_ok / cenc_sample_ok what the calls refuse -- and the
 * host-visible launchers.  Everything above the device part compiles with plain g++ (tests/test_cenc_host_asan.py
 * single-steps both plans and the block function with it).
 *
 * AES words are big-endian: word i of a block is bytes 4 i .. 4 i + 3, the first on top.  Te0[x] = (2 S[x], S[x], S[x], 3 S[x]);
 * the other three tables of the usual formulation are byte rotations of it, and S[x] itself is its second byte.
 */
#ifndef HBS_CENC_H
#define HBS_CENC_H

#include "hbs_common.h"

namespace hbs {

constexpr uint64_t kCencMaxClear = 65535;             /* the 16-bit clear count of a senc entry                       */
constexpr uint64_t kCencMaxEntries = 1ull << 48;      /* d_sub_first values at or above this are refused              */
constexpr int kCencNalsPer = 8;                       /* plan: consecutive NALs a lane takes                          */
constexpr int kCencNalsPerBlock = 256 * kCencNalsPer;
constexpr uint32_t kCencRanges = 1024;                /* crypt: the entries are walked in this many equal ranges      */
constexpr uint64_t kCencTileBytes = 64 * 1024;        /* crypt: protected bytes of one workgroup                      */

/* ---- AES-128 ------------------------------------------------------------------------------------------------------------- */

HBS_HD uint32_t cenc_sbox(uint32_t x)
{
    static constexpr uint8_t s[256] = {
        0x63, 0x7c, 0x77, 0x7b, 0xf2, 0x6b, 0x6f, 0xc5, 0x30, 0x01, 0x67, 0x2b, 0xfe, 0xd7, 0xab, 0x76,
        0xca, 0x82, 0xc9, 0x7d, 0xfa, 0x59, 0x47, 0xf0, 0xad, 0xd4, 0xa2, 0xaf, 0x9c, 0xa4, 0x72, 0xc0,
        0xb7, 0xfd, 0x93, 0x26, 0x36, 0x3f, 0xf7, 0xcc, 0x34, 0xa5, 0xe5, 0xf1, 0x71, 0xd8, 0x31, 0x15,
        0x04, 0xc7, 0x23, 0xc3, 0x18, 0x96, 0x05, 0x9a, 0x07, 0x12, 0x80, 0xe2, 0xeb, 0x27, 0xb2, 0x75,
        0x09, 0x83, 0x2c, 0x1a, 0x1b, 0x6e, 0x5a, 0xa0, 0x52, 0x3b, 0xd6, 0xb3, 0x29, 0xe3, 0x2f, 0x84,
        0x53, 0xd1, 0x00, 0xed, 0x20, 0xfc, 0xb1, 0x5b, 0x6a, 0xcb, 0xbe, 0x39, 0x4a, 0x4c, 0x58, 0xcf,
        0xd0, 0xef, 0xaa, 0xfb, 0x43, 0x4d, 0x33, 0x85, 0x45, 0xf9, 0x02, 0x7f, 0x50, 0x3c, 0x9f, 0xa8,
        0x51, 0xa3, 0x40, 0x8f, 0x92, 0x9d, 0x38, 0xf5, 0xbc, 0xb6, 0xda, 0x21, 0x10, 0xff, 0xf3, 0xd2,
        0xcd, 0x0c, 0x13, 0xec, 0x5f, 0x97, 0x44, 0x17, 0xc4, 0xa7, 0x7e, 0x3d, 0x64, 0x5d, 0x19, 0x73,
        0x60, 0x81, 0x4f, 0xdc, 0x22, 0x2a, 0x90, 0x88, 0x46, 0xee, 0xb8, 0x14, 0xde, 0x5e, 0x0b, 0xdb,
        0xe0, 0x32, 0x3a, 0x0a, 0x49, 0x06, 0x24, 0x5c, 0xc2, 0xd3, 0xac, 0x62, 0x91, 0x95, 0xe4, 0x79,
        0xe7, 0xc8, 0x37, 0x6d, 0x8d, 0xd5, 0x4e, 0xa9, 0x6c, 0x56, 0xf4, 0xea, 0x65, 0x7a, 0xae, 0x08,
        0xba, 0x78, 0x25, 0x2e, 0x1c, 0xa6, 0xb4, 0xc6, 0xe8, 0xdd, 0x74, 0x1f, 0x4b, 0xbd, 0x8b, 0x8a,
        0x70, 0x3e, 0xb5, 0x66, 0x48, 0x03, 0xf6, 0x0e, 0x61, 0x35, 0x57, 0xb9, 0x86, 0xc1, 0x1d, 0x9e,
        0xe1, 0xf8, 0x98, 0x11, 0x69, 0xd9, 0x8e, 0x94, 0x9b, 0x1e, 0x87, 0xe9, 0xce, 0x55, 0x28, 0xdf,
        0x8c, 0xa1, 0x89, 0x0d, 0xbf, 0xe6, 0x42, 0x68, 0x41, 0x99, 0x2d, 0x0f, 0xb0, 0x54, 0xbb, 0x16};
    return s[x & 0xFFu];
}

HBS_HD uint32_t cenc_xtime(uint32_t b) { return ((b << 1) ^ ((b & 0x80u) ? 0x1Bu : 0u)) & 0xFFu; }
HBS_HD uint32_t cenc_te0(uint32_t x)
{
    const uint32_t s = cenc_sbox(x), s2 = cenc_xtime(s);
    return (s2 << 24) | (s << 16) | (s << 8) | (s2 ^ s);
}
HBS_HD uint32_t cenc_ror(uint32_t v, uint32_t n) { return (v >> n) | (v << (32u - n)); }      /* n in 8, 16, 24 */

struct CencKey { uint32_t rk[44]; };                  /* the 11 round keys: 176 bytes, passed to the kernels by value */

HBS_HD void cenc_expand_key(const uint8_t key[16], CencKey& k)
{
    for (int i = 0; i < 4; ++i)
        k.rk[i] = ((uint32_t)key[4 * i] << 24) | ((uint32_t)key[4 * i + 1] << 16) | ((uint32_t)key[4 * i + 2] << 8) | key[4 * i + 3];
    uint32_t rcon = 1;
    for (int i = 4; i < 44; ++i) {
        uint32_t t = k.rk[i - 1];
        if ((i & 3) == 0) {
            t = (t << 8) | (t >> 24);
            t = (cenc_sbox(t >> 24) << 24) | (cenc_sbox((t >> 16) & 0xFFu) << 16) | (cenc_sbox((t >> 8) & 0xFFu) << 8) | cenc_sbox(t & 0xFFu);
            t ^= rcon << 24;
            rcon = cenc_xtime(rcon);
        }
        k.rk[i] = k.rk[i - 4] ^ t;
    }
}

/* one block: out = AES-128_k(in), words big-endian.  te0(x) gives Te0[x]: from LDS in the kernel, cenc_te0 itself on the host */
template <class Te0>
HBS_HD void cenc_aes_block(const CencKey& k, const uint32_t in[4], uint32_t out[4], Te0 te0)
{
    uint32_t s0 = in[0] ^ k.rk[0], s1 = in[1] ^ k.rk[1], s2 = in[2] ^ k.rk[2], s3 = in[3] ^ k.rk[3];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 1; r < 10; ++r) {
        const uint32_t t0 = te0(s0 >> 24) ^ cenc_ror(te0((s1 >> 16) & 0xFFu), 8) ^ cenc_ror(te0((s2 >> 8) & 0xFFu), 16) ^ cenc_ror(te0(s3 & 0xFFu), 24) ^ k.rk[4 * r];
        const uint32_t t1 = te0(s1 >> 24) ^ cenc_ror(te0((s2 >> 16) & 0xFFu), 8) ^ cenc_ror(te0((s3 >> 8) & 0xFFu), 16) ^ cenc_ror(te0(s0 & 0xFFu), 24) ^ k.rk[4 * r + 1];
        const uint32_t t2 = te0(s2 >> 24) ^ cenc_ror(te0((s3 >> 16) & 0xFFu), 8) ^ cenc_ror(te0((s0 >> 8) & 0xFFu), 16) ^ cenc_ror(te0(s1 & 0xFFu), 24) ^ k.rk[4 * r + 2];
        const uint32_t t3 = te0(s3 >> 24) ^ cenc_ror(te0((s0 >> 16) & 0xFFu), 8) ^ cenc_ror(te0((s1 >> 8) & 0xFFu), 16) ^ cenc_ror(te0(s2 & 0xFFu), 24) ^ k.rk[4 * r + 3];
        s0 = t0; s1 = t1; s2 = t2; s3 = t3;
    }
    /* the last round has no MixColumns: S[x] is the second byte of Te0[x] */
#define HBS_CENC_SB(x) ((te0(x) >> 8) & 0xFFu)
    out[0] = ((HBS_CENC_SB(s0 >> 24) << 24) | (HBS_CENC_SB((s1 >> 16) & 0xFFu) << 16) | (HBS_CENC_SB((s2 >> 8) & 0xFFu) << 8) | HBS_CENC_SB(s3 & 0xFFu)) ^ k.rk[40];
    out[1] = ((HBS_CENC_SB(s1 >> 24) << 24) | (HBS_CENC_SB((s2 >> 16) & 0xFFu) << 16) | (HBS_CENC_SB((s3 >> 8) & 0xFFu) << 8) | HBS_CENC_SB(s0 & 0xFFu)) ^ k.rk[41];
    out[2] = ((HBS_CENC_SB(s2 >> 24) << 24) | (HBS_CENC_SB((s3 >> 16) & 0xFFu) << 16) | (HBS_CENC_SB((s0 >> 8) & 0xFFu) << 8) | HBS_CENC_SB(s1 & 0xFFu)) ^ k.rk[42];
    out[3] = ((HBS_CENC_SB(s3 >> 24) << 24) | (HBS_CENC_SB((s0 >> 16) & 0xFFu) << 16) | (HBS_CENC_SB((s1 >> 8) & 0xFFu) << 8) | HBS_CENC_SB(s2 & 0xFFu)) ^ k.rk[43];
#undef HBS_CENC_SB
}

/* byte q (0..15) of a block of big-endian words */
HBS_HD uint32_t cenc_block_byte(const uint32_t w[4], uint32_t q) { return (w[q >> 2] >> (24u - 8u * (q & 3u))) & 0xFFu; }

/* ---- the counter ---------------------------------------------------------------------------------------------------------- */

struct CencCtr { uint64_t hi, lo; };                  /* bytes 0..7 and 8..15 of a sample's counter block, big-endian */

HBS_HD uint64_t cenc_be64(const uint8_t* p)
{
    uint64_t v = 0;
    for (int i = 0; i < 8; ++i) v = (v << 8) | p[i];
    return v;
}
HBS_HD CencCtr cenc_ctr_load(const uint8_t* iv16) { CencCtr c; c.hi = cenc_be64(iv16); c.lo = cenc_be64(iv16 + 8); return c; }
/* iv_mode 1: iv_base = the big-endian value of iv0[0..8); sample s counts from (iv_base + s mod 2^64) : 0 */
HBS_HD CencCtr cenc_ctr_seq(uint64_t iv_base, uint64_t s) { CencCtr c; c.hi = iv_base + s; c.lo = 0; return c; }
HBS_HD void cenc_ctr_store(const CencCtr& c, uint8_t* out16)
{
    for (int i = 0; i < 8; ++i) { out16[i] = (uint8_t)(c.hi >> (56 - 8 * i)); out16[8 + i] = (uint8_t)(c.lo >> (56 - 8 * i)); }
}
/* the counter block of keystream block j of the sample: the addition wraps inside bytes 8..15, nothing carries into 0..7 */
HBS_HD void cenc_ctr_block(const CencCtr& c, uint64_t j, uint32_t in[4])
{
    const uint64_t lo = c.lo + j;
    in[0] = (uint32_t)(c.hi >> 32); in[1] = (uint32_t)c.hi; in[2] = (uint32_t)(lo >> 32); in[3] = (uint32_t)lo;
}

/* ---- the subsample rule ---------------------------------------------------------------------------------------------------- */

HBS_HD bool cenc_plan_params_ok(const hbs_cenc_plan_params* p)
{
    if (!p || (p->length_size != 1 && p->length_size != 2 && p->length_size != 4)) return false;
    return (p->flags & ~HBS_CENC_ALIGN16) == 0u && p->reserved == 0u && p->clear_lead >= 2u;
}
HBS_HD bool cenc_params_ok(const hbs_cenc_params* p)
{
    return p && p->scheme == HBS_CENC_SCHEME_CENC && p->iv_mode <= 1u && p->flags == 0u && p->reserved == 0u;
}

struct CencNal { uint64_t clear, protect; bool bad; };       /* what a kept NAL adds to the running clear count, then protects */

/* a kept NAL [start, end) whose first payload byte gives `type` (not looked at for an empty NAL): L length bytes and the clear
 * lead stay clear.  have_off: payload_off is d_payload_off[k] */
HBS_HD CencNal cenc_nal_split(uint32_t L, uint64_t start, uint64_t end, uint32_t type, bool have_off, uint64_t payload_off,
                              uint32_t clear_lead, uint32_t flags)
{
    CencNal r;
    const uint64_t size = end - start;
    r.bad = false; r.protect = 0; r.clear = L + size;
    if (size == 0 || type >= 32u) return r;
    uint64_t h;
    if (have_off) {
        if (payload_off == ~0ull || payload_off < start + 2u || payload_off > end) { r.bad = true; return r; }
        h = payload_off - start;
    } else {
        h = clear_lead < size ? clear_lead : size;
    }
    uint64_t P = size - h;
    if (flags & HBS_CENC_ALIGN16) { h += P & 15u; P &= ~15ull; }
    r.clear = L + h; r.protect = P;
    return r;
}

/* the entries that (C, P) becomes: max(ceil(C / 65535), 1) */
HBS_HD uint64_t cenc_entries(uint64_t C) { return C <= kCencMaxClear ? 1u : (C + kCencMaxClear - 1u) / kCencMaxClear; }
/* entry i of the cnt = cenc_entries(C) entries of (C, P) */
HBS_HD hbs_cenc_subsample cenc_entry(uint64_t C, uint64_t P, uint64_t i, uint64_t cnt)
{
    hbs_cenc_subsample e;
    if (i + 1 < cnt) { e.clear = (uint32_t)kCencMaxClear; e.protect = 0; }
    else { e.clear = (uint32_t)(C - kCencMaxClear * (cnt - 1u)); e.protect = (uint32_t)P; }
    return e;
}
/* the entries NAL k leaves: R = the running clear count with the NAL's own clear bytes in it, P its protected bytes (0: none,
 * or not kept), last_of_au: no NAL of its AU follows.  A protected range ends a run; so does the sample's end, if anything is left */
HBS_HD uint64_t cenc_nal_entries(uint64_t R, uint64_t P, bool last_of_au) { return P ? cenc_entries(R) : (last_of_au && R) ? cenc_entries(R) : 0u; }

/* ---- hbs_cenc_crypt's checks ---------------------------------------------------------------------------------------------- */

/* what is about sample s alone: it lies in the buffer, in front of the next one (has_next), and d_sub_first rises from 0 */
HBS_HD bool cenc_sample_ok(uint64_t s, uint64_t off, uint64_t size, bool has_next, uint64_t next_off, uint64_t data_bytes,
                           uint64_t first, uint64_t first_next)
{
    if (off > data_bytes || size > data_bytes - off) return false;
    if (has_next && off + size > next_off) return false;
    if (first > first_next || first_next >= kCencMaxEntries) return false;
    return s != 0 || first == 0;
}

/* the entries [lo, hi) of range g of G over E entries */
HBS_HD uint64_t cenc_range_begin(uint64_t E, uint32_t g, uint32_t G) { return E / G * g + E % G * g / G; }

} // namespace hbs

#ifdef __HIPCC__
#include <hip/hip_runtime_api.h>
namespace hbs {


struct CencPlanArgs {
    const uint8_t* src; uint64_t n;
    const hbs_nal_entry* index; uint64_t n_nals;
    const uint8_t* keep;
    const uint32_t* nal_au; uint64_t n_aus;
    const unsigned long long* payload_off;            /* nullable                                                     */
    uint32_t L, flags, clear_lead;
    unsigned long long* sub_first; hbs_cenc_subsample* sub; uint64_t sub_cap;
    hbs_summary* summary;
    /* scratch (lay_cenc_plan): 128 bytes per 2 048 NALs */
    unsigned long long* part_a;     /* 8 per plan block: the clear count its last run ends with -> the one its first lane continues;
                                       whether a run begins in it; 1 + its lowest bad NAL */
    unsigned long long* part_b;     /* 8 per plan block: entries, protected bytes, sample bytes, kept NALs; 1 + its lowest bad NAL */
    unsigned long long* ctl;        /* 8: the error                                                                  */
    hipEvent_t ev_begin, ev_end;
};
inline void lay_cenc_plan(Carver& w, CencPlanArgs& a)
{
    const uint64_t blocks = (a.n_nals + kCencNalsPerBlock - 1) / kCencNalsPerBlock;
    a.part_a = w.take<unsigned long long>(blocks * 64);
    a.part_b = w.take<unsigned long long>(blocks * 64);
    a.ctl = w.take<unsigned long long>(64);
}
hipError_t launch_cenc_subsamples(const CencPlanArgs& a, hipStream_t st);

struct CencArgs {
    uint8_t* data; uint64_t n;
    const unsigned long long* sample_off; const unsigned long long* sample_size; uint64_t n_samples;
    const unsigned long long* sub_first; const hbs_cenc_subsample* sub;
    uint8_t* iv;                                      /* iv_mode 0: read; 1: written when non-null                    */
    uint32_t iv_mode; uint64_t iv_base;
    hbs_summary* summary;
    /* scratch (lay_cenc): 16 bytes a sample, 64 bytes per 256 samples, 64 a range -- nothing of it depends on the key */
    unsigned long long* at_b;       /* n_samples + 1: the bytes of all entries in front of the sample's first               */
    unsigned long long* at_k;       /* n_samples + 1: ... the protected bytes of them                                       */
    unsigned long long* part_s;     /* 8 per 256 samples: 1 + the lowest bad sample                                         */
    unsigned long long* part_r;     /* 8 a range (+ 8): bytes, protected bytes -> those in front of it; 1 + the lowest bad sample */
    unsigned long long* ctl;        /* 8: kCencC*                                                                           */
    uint64_t tiles;                 /* the crypt kernel's grid                                                              */
    hipEvent_t ev_begin, ev_end;
};
enum : int { kCencCErr = 0, kCencCEntries = 1, kCencCProt = 2, kCencCBad = 3 };
/* what the host hands to the launcher: the round keys go with the crypt kernel's launch, by value, never into scratch */
struct CencCall : CencArgs { CencKey key; };
inline void lay_cenc_args(Carver& w, CencArgs& a)       /* (hbs_cbcs_crypt carves the same: hbs_cbcs.h) */
{
    a.at_b = w.take<unsigned long long>((a.n_samples + 1) * 8);
    a.at_k = w.take<unsigned long long>((a.n_samples + 1) * 8);
    a.part_s = w.take<unsigned long long>((a.n_samples + 255) / 256 * 64);
    a.part_r = w.take<unsigned long long>(((uint64_t)kCencRanges + 1) * 64);
    a.ctl = w.take<unsigned long long>(64);
}
inline void lay_cenc(Carver& w, CencCall& a) { lay_cenc_args(w, a); }
hipError_t launch_cenc_crypt(const CencCall& c, hipStream_t st);
/* the checks of hbs_cenc_crypt alone, k_cenc_samples to k_cenc_verdict: at_b, at_k, part_r, ctl and the summary (with rbsp_bytes
 * = the protected bytes) are as the crypt kernel finds them; no events.  hbs_cbcs_crypt begins with them too */
void enqueue_cenc_checks(const CencArgs& a, hipStream_t st);

} // namespace hbs
#endif
#endif
