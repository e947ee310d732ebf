/*
 * hbs_cbcs.h -- hbs_cbcs_crypt (include/hevcbitstream_amd.h): the rules as host/device inline functions -- cbcs_inv_sbox /
 * cbcs_td0_of / cbcs_expand_dec_key / cbcs_aes_inv_block are the equivalent inverse cipher of AES-128 (FIPS-197 5.3.5) over one
 * table of 256 words and the inverse S-box, cbcs_pattern / cbcs_is_crypt / cbcs_crypt_blocks / cbcs_block_of the block pattern
 * of ISO/IEC 23001-7 `cbcs`, cbcs_params_ok what the call refuses -- and the host-visible launcher.  The forward cipher, the
 * samples' checks and the scratch are hbs_cenc.h's.  Everything above the device part compiles with plain g++
 * (tests/test_cbcs_host_asan.py single-steps it).
 *
 * There is no second literal table: the inverse S-box is read off cenc_sbox (inv[S[x]] = x), and Td0[x] = (14, 9, 13, 11) .
 * inv[x], big-endian like Te0; the other three tables of the usual formulation are byte rotations of it.
 */
#ifndef HBS_CBCS_H
#define HBS_CBCS_H

#include "hbs_cenc.h"

namespace hbs {

constexpr uint32_t kCbcsLaneBlocks = 64;              /* decrypt: an entry of fewer crypt blocks than this is one lane's loop,
                                                         a longer one a wavefront's (the wavefront's width)               */

/* ---- the inverse cipher ---------------------------------------------------------------------------------------------------- */

/* the y with S[y] == x, by search: for the host (the kernel fills its table the other way round, a lane an x) */
HBS_HD uint32_t cbcs_inv_sbox(uint32_t x)
{
    uint32_t y = 0;
    while (cenc_sbox(y) != (x & 0xFFu)) y += 1;
    return y;
}

/* (14 v, 9 v, 13 v, 11 v) in GF(2^8), the first on top: Td0[x] = cbcs_td0_of(inv[x]) */
HBS_HD uint32_t cbcs_td0_of(uint32_t v)
{
    const uint32_t v2 = cenc_xtime(v), v4 = cenc_xtime(v2), v8 = cenc_xtime(v4);
    return ((v8 ^ v4 ^ v2) << 24) | ((v8 ^ v) << 16) | ((v8 ^ v4 ^ v) << 8) | (v8 ^ v2 ^ v);
}

/* InvMixColumns of one column (a big-endian word) */
HBS_HD uint32_t cbcs_inv_mix(uint32_t w)
{
    return cbcs_td0_of(w >> 24) ^ cenc_ror(cbcs_td0_of((w >> 16) & 0xFFu), 8) ^ cenc_ror(cbcs_td0_of((w >> 8) & 0xFFu), 16) ^
           cenc_ror(cbcs_td0_of(w & 0xFFu), 24);
}

/* the round keys of the equivalent inverse cipher: those of the cipher in reverse order, InvMixColumns on rounds 1..9 */
HBS_HD void cbcs_expand_dec_key(const CencKey& ek, CencKey& dk)
{
    for (int r = 0; r <= 10; ++r)
        for (int j = 0; j < 4; ++j) {
            const uint32_t w = ek.rk[4 * (10 - r) + j];
            dk.rk[4 * r + j] = (r == 0 || r == 10) ? w : cbcs_inv_mix(w);
        }
}

/* one block: out = AES-128^-1(in), words big-endian, dk from cbcs_expand_dec_key.  td0(x) gives Td0[x], inv(x) the inverse
 * S-box: from LDS in the kernel; cbcs_td0_of(cbcs_inv_sbox(x)) and cbcs_inv_sbox on the host */
template <class Td0, class Inv>
HBS_HD void cbcs_aes_inv_block(const CencKey& dk, const uint32_t in[4], uint32_t out[4], Td0 td0, Inv inv)
{
    uint32_t s0 = in[0] ^ dk.rk[0], s1 = in[1] ^ dk.rk[1], s2 = in[2] ^ dk.rk[2], s3 = in[3] ^ dk.rk[3];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 1; r < 10; ++r) {
        const uint32_t t0 = td0(s0 >> 24) ^ cenc_ror(td0((s3 >> 16) & 0xFFu), 8) ^ cenc_ror(td0((s2 >> 8) & 0xFFu), 16) ^ cenc_ror(td0(s1 & 0xFFu), 24) ^ dk.rk[4 * r];
        const uint32_t t1 = td0(s1 >> 24) ^ cenc_ror(td0((s0 >> 16) & 0xFFu), 8) ^ cenc_ror(td0((s3 >> 8) & 0xFFu), 16) ^ cenc_ror(td0(s2 & 0xFFu), 24) ^ dk.rk[4 * r + 1];
        const uint32_t t2 = td0(s2 >> 24) ^ cenc_ror(td0((s1 >> 16) & 0xFFu), 8) ^ cenc_ror(td0((s0 >> 8) & 0xFFu), 16) ^ cenc_ror(td0(s3 & 0xFFu), 24) ^ dk.rk[4 * r + 2];
        const uint32_t t3 = td0(s3 >> 24) ^ cenc_ror(td0((s2 >> 16) & 0xFFu), 8) ^ cenc_ror(td0((s1 >> 8) & 0xFFu), 16) ^ cenc_ror(td0(s0 & 0xFFu), 24) ^ dk.rk[4 * r + 3];
        s0 = t0; s1 = t1; s2 = t2; s3 = t3;
    }
    /* the last round has no InvMixColumns */
    out[0] = ((inv(s0 >> 24) << 24) | (inv((s3 >> 16) & 0xFFu) << 16) | (inv((s2 >> 8) & 0xFFu) << 8) | inv(s1 & 0xFFu)) ^ dk.rk[40];
    out[1] = ((inv(s1 >> 24) << 24) | (inv((s0 >> 16) & 0xFFu) << 16) | (inv((s3 >> 8) & 0xFFu) << 8) | inv(s2 & 0xFFu)) ^ dk.rk[41];
    out[2] = ((inv(s2 >> 24) << 24) | (inv((s1 >> 16) & 0xFFu) << 16) | (inv((s0 >> 8) & 0xFFu) << 8) | inv(s3 & 0xFFu)) ^ dk.rk[42];
    out[3] = ((inv(s3 >> 24) << 24) | (inv((s2 >> 16) & 0xFFu) << 16) | (inv((s1 >> 8) & 0xFFu) << 8) | inv(s0 & 0xFFu)) ^ dk.rk[43];
}

/* ---- the pattern ----------------------------------------------------------------------------------------------------------- */

struct CbcsPattern { uint32_t c, k, whole; };         /* c >= 1; whole: HBS_CBCS_WHOLE_RUNS                           */

/* crypt_byte_block, skip_byte_block (both 0: every block) and the flags of a params record that cbcs_params_ok passed */
HBS_HD CbcsPattern cbcs_pattern(uint32_t crypt_byte_block, uint32_t skip_byte_block, uint32_t flags)
{
    CbcsPattern p;
    p.c = crypt_byte_block ? crypt_byte_block : 1u;
    p.k = crypt_byte_block ? skip_byte_block : 0u;
    p.whole = (flags & HBS_CBCS_WHOLE_RUNS) ? 1u : 0u;
    return p;
}
/* block i of the nb whole blocks of a protected range is a crypt block */
HBS_HD bool cbcs_is_crypt(const CbcsPattern& p, uint32_t nb, uint32_t i)
{
    const uint32_t r = i % (p.c + p.k);
    return i < nb && r < p.c && (!p.whole || i - r + p.c <= nb);
}
/* the crypt blocks among nb whole blocks */
HBS_HD uint32_t cbcs_crypt_blocks(const CbcsPattern& p, uint32_t nb)
{
    const uint32_t f = nb / (p.c + p.k), m = nb % (p.c + p.k);
    return f * p.c + (p.whole ? (m >= p.c ? p.c : 0u) : (m < p.c ? m : p.c));
}
/* the block that is the j-th crypt block */
HBS_HD uint32_t cbcs_block_of(const CbcsPattern& p, uint32_t j) { return j / p.c * (p.c + p.k) + j % p.c; }

HBS_HD bool cbcs_params_ok(const hbs_cbcs_params* p)
{
    if (!p || p->iv_mode > 1u || (p->flags & ~(HBS_CBCS_DECRYPT | HBS_CBCS_WHOLE_RUNS)) != 0u) return false;
    if (p->crypt_byte_block > 15u || p->skip_byte_block > 15u || (p->crypt_byte_block == 0u && p->skip_byte_block != 0u)) return false;
    return p->reserved0 == 0u && p->reserved1 == 0u;
}

/* the big-endian words of a 16-byte block */
HBS_HD void cbcs_load_be(const uint8_t b[16], uint32_t w[4])
{
    for (int i = 0; i < 4; ++i) w[i] = ((uint32_t)b[4 * i] << 24) | ((uint32_t)b[4 * i + 1] << 16) | ((uint32_t)b[4 * i + 2] << 8) | b[4 * i + 3];
}

} // namespace hbs

#ifdef __HIPCC__
namespace hbs {

/* what the host hands to the launcher.  The samples, the tables and the scratch are hbs_cenc_crypt's (CencArgs, lay_cenc: `tiles`
 * and `iv_base` are not used, `iv` is only read); the round keys of the direction and iv0 go with the crypt kernel's launch, by
 * value, never into scratch.  The crypt kernel leaves the crypt blocks of range g in part_r[8 g + 3]. */
struct CbcsCall : CencArgs {
    CbcsPattern pattern;
    uint32_t decrypt;
    uint32_t iv0[4];                /* iv_mode 1: the IV of every sample, big-endian words                                   */
    CencKey ek, dk;                 /* the cipher's round keys, the equivalent inverse cipher's                              */
};
enum : int { kCbcsRBlocks = 3 };    /* the word of a range's 8 in part_r                                                     */
inline void lay_cbcs(Carver& w, CbcsCall& a) { lay_cenc_args(w, a); }
hipError_t launch_cbcs_crypt(const CbcsCall& c, hipStream_t st);

} // namespace hbs
#endif
#endif
