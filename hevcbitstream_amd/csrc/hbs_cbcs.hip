/*
 * hbs_cbcs.hip -- hbs_cbcs_crypt: AES-128-CBC in place over the crypt blocks of every protected range, ISO/IEC 23001-7 `cbcs`
 * (include/hevcbitstream_amd.h is the specification, hbs_cbcs.h the rules).  No launch waits for another workgroup.
 *
 *   enqueue_cenc_checks   hbs_cenc_crypt's own seven launches (hbs_cenc.hip), unchanged: every check, the bytes in front of every
 *                    range of entries (part_r) and of every sample's first entry (at_b), the error, the summary
 *   k_cbcs_crypt     a workgroup per range of entries, 256 entries a step; instantiated per direction.  A block scan gives the
 *                    place of each entry's protected range, a search of d_sub_first its sample (for the IV and the sample's
 *                    offset).  The lane then walks the entry's crypt blocks itself: a 16-byte load at the block's own byte
 *                    address, XOR, cipher, store, the previous ciphertext block in registers.  In place this has no hazard in
 *                    either direction.  When decrypting, an entry of kCbcsLaneBlocks crypt blocks or more goes to a list in LDS
 *                    instead, and behind a barrier the workgroup's wavefronts take the listed entries in turn, 64 consecutive
 *                    crypt blocks a step: every lane loads its own ciphertext block, takes the previous one from the lane below
 *                    (lane 0: the last step's lane 63, or the IV), deciphers, XORs, stores.  All loads of a step come before its
 *                    stores in the one wavefront's program order and the steps are disjoint, and no other wavefront touches
 *                    the entry: no barrier and no second buffer.  A long entry that is ENCRYPTED stays on its lane: C_j needs
 *                    C_(j-1).  Nothing but crypt blocks is stored.  The crypt blocks of the range go to part_r[8 g + 3]
 *   k_cbcs_summary   one workgroup: rbsp_bytes = 16 x their sum
 * AES: Te0 (encrypt) or Td0 and the inverse S-box (decrypt) in LDS, filled once a workgroup -- lane x writes inv[S[x]] = x, then
 * Td0[x] from inv[x]; the round keys of the direction are a kernel argument.
 */
#include <hip/hip_runtime.h>
#include "hbs_cbcs.h"
#include "hbs_plan.h"
#include "hbs_copy16.h"

namespace hbs {
namespace {

constexpr int kT = kPlanLanes;
constexpr int kWaves = kT / 64;
static_assert(kCbcsLaneBlocks >= 1, "an entry without crypt blocks is nobody's");

struct CbcsKernelArgs { CbcsPattern pattern; uint32_t iv0[4]; };

/* the 16 bytes at any address as big-endian words, and back */
__device__ __forceinline__ void load_block(const uint8_t* p, uint32_t w[4])
{
    const u32x4 d = *reinterpret_cast<const u32x4_u1*>(p);
    w[0] = __builtin_bswap32(d.x); w[1] = __builtin_bswap32(d.y); w[2] = __builtin_bswap32(d.z); w[3] = __builtin_bswap32(d.w);
}
__device__ __forceinline__ void store_block(uint8_t* p, const uint32_t w[4])
{
    u32x4 d;
    d.x = __builtin_bswap32(w[0]); d.y = __builtin_bswap32(w[1]); d.z = __builtin_bswap32(w[2]); d.w = __builtin_bswap32(w[3]);
    *reinterpret_cast<u32x4_u1*>(p) = d;
}

/* sample s's IV */
__device__ __forceinline__ void sample_iv(const CencArgs& a, const CbcsKernelArgs& k, uint64_t s, uint32_t iv[4])
{
    if (a.iv_mode) { iv[0] = k.iv0[0]; iv[1] = k.iv0[1]; iv[2] = k.iv0[2]; iv[3] = k.iv0[3]; return; }
    const uint32_t* w = reinterpret_cast<const uint32_t*>(a.iv + 16 * s);
    iv[0] = __builtin_bswap32(w[0]); iv[1] = __builtin_bswap32(w[1]); iv[2] = __builtin_bswap32(w[2]); iv[3] = __builtin_bswap32(w[3]);
}

/* one lane, one entry: its n crypt blocks from p on, in order */
template <bool kDec, class Tab, class Inv>
__device__ __forceinline__ void chain_lane(uint8_t* p, uint32_t n, const CbcsPattern& pat, const uint32_t iv[4], const CencKey& key, Tab tab, Inv inv)
{
    uint32_t prev[4] = {iv[0], iv[1], iv[2], iv[3]};
    uint32_t r = 0;                                    /* the crypt blocks of the run so far */
#pragma unroll 1
    for (uint32_t j = 0; j < n; ++j) {
        uint32_t x[4], y[4];
        load_block(p, x);
        if constexpr (kDec) {
            cbcs_aes_inv_block(key, x, y, tab, inv);
            y[0] ^= prev[0]; y[1] ^= prev[1]; y[2] ^= prev[2]; y[3] ^= prev[3];
            prev[0] = x[0]; prev[1] = x[1]; prev[2] = x[2]; prev[3] = x[3];
        } else {
            x[0] ^= prev[0]; x[1] ^= prev[1]; x[2] ^= prev[2]; x[3] ^= prev[3];
            cenc_aes_block(key, x, y, tab);
            prev[0] = y[0]; prev[1] = y[1]; prev[2] = y[2]; prev[3] = y[3];
        }
        store_block(p, y);
        p += 16; r += 1;
        if (r == pat.c) { r = 0; p += 16u * pat.k; }
    }
}

/* one wavefront, one entry, decrypting: p, n and iv are the same in every lane */
template <class Tab, class Inv>
__device__ __forceinline__ void chain_wave(uint8_t* p, uint32_t n, const CbcsPattern& pat, const uint32_t iv[4], const CencKey& key, Tab tab, Inv inv)
{
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t carry[4] = {iv[0], iv[1], iv[2], iv[3]};
#pragma unroll 1
    for (uint32_t base = 0; base < n; base += 64u) {
        const uint32_t j = base + lane;
        const bool on = j < n;
        uint8_t* q = p + 16ull * cbcs_block_of(pat, on ? j : base);
        uint32_t x[4] = {0, 0, 0, 0}, prev[4], y[4];
        if (on) load_block(q, x);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t up = __shfl_up(x[i], 1u, 64);
            prev[i] = lane ? up : carry[i];
            carry[i] = __shfl(x[i], 63, 64);
        }
        if (on) {
            cbcs_aes_inv_block(key, x, y, tab, inv);
            y[0] ^= prev[0]; y[1] ^= prev[1]; y[2] ^= prev[2]; y[3] ^= prev[3];
            store_block(q, y);
        }
    }
}

template <bool kDec>
__global__ __launch_bounds__(kT) void k_cbcs_crypt(CencArgs a, CbcsKernelArgs k, CencKey key)
{
    __shared__ uint32_t s_tab[256];                    /* Te0, or Td0 */
    __shared__ uint8_t s_inv[kDec ? 256 : 4];
    __shared__ unsigned long long s_lpos[kDec ? kT : 1];
    __shared__ uint32_t s_ln[kDec ? kT : 1], s_ls[kDec ? kT : 1], s_nlong;
    if (a.ctl[kCencCErr] != 0) return;
    static_assert(kT == 256, "a lane fills one word of the table");
    if constexpr (kDec) {
        s_inv[cenc_sbox(threadIdx.x)] = (uint8_t)threadIdx.x;
        __syncthreads();
        s_tab[threadIdx.x] = cbcs_td0_of(s_inv[threadIdx.x]);
    } else {
        s_tab[threadIdx.x] = cenc_te0(threadIdx.x);
    }
    const auto tab = [&](uint32_t x) { return s_tab[x]; };
    const auto inv = [&](uint32_t x) { return (uint32_t)s_inv[x]; };
    const CbcsPattern pat = k.pattern;
    const uint64_t E = a.ctl[kCencCEntries];
    const uint64_t lo = cenc_range_begin(E, blockIdx.x, kCencRanges), hi = cenc_range_begin(E, blockIdx.x + 1, kCencRanges);
    uint64_t Bc = a.part_r[(uint64_t)blockIdx.x * 8];
    uint64_t done = 0;
    __syncthreads();
#pragma unroll 1
    for (uint64_t e0 = lo; e0 < hi; e0 += kT) {
        const uint32_t cnt = hi - e0 < (uint64_t)kT ? (uint32_t)(hi - e0) : (uint32_t)kT;
        if (threadIdx.x == 0) s_nlong = 0;
        hbs_cenc_subsample x;
        x.clear = 0; x.protect = 0;
        if (threadIdx.x < cnt) x = a.sub[e0 + threadIdx.x];
        uint64_t v = (uint64_t)x.clear + x.protect, ex, tot;
        block_scan<1, kT>(&v, &ex, &tot);
        const uint32_t n = cbcs_crypt_blocks(pat, x.protect >> 4);
        if (n) {
            done += n;
            const uint64_t e = e0 + threadIdx.x;
            const uint64_t s = last_le((uint64_t)0, a.n_samples - 1, e, [&](uint64_t i) { return (uint64_t)a.sub_first[i]; });
            const uint64_t pos = a.sample_off[s] + (Bc + ex - a.at_b[s]) + x.clear;
            bool mine = true;
            if constexpr (kDec) {
                if (n >= kCbcsLaneBlocks) {
                    const uint32_t at = atomicAdd(&s_nlong, 1u);
                    s_lpos[at] = pos; s_ln[at] = n; s_ls[at] = (uint32_t)s;
                    mine = false;
                }
            }
            if (mine) {
                uint32_t iv[4];
                sample_iv(a, k, s, iv);
                chain_lane<kDec>(a.data + pos, n, pat, iv, key, tab, inv);
            }
        }
        if constexpr (kDec) {
            __syncthreads();
            const uint32_t listed = __builtin_amdgcn_readfirstlane(s_nlong);
#pragma unroll 1
            for (uint32_t i = threadIdx.x >> 6; i < listed; i += kWaves) {
                uint32_t iv[4];
                sample_iv(a, k, s_ls[i], iv);
                chain_wave(a.data + s_lpos[i], s_ln[i], pat, iv, key, tab, inv);
            }
            __syncthreads();
        }
        Bc += tot;
    }
    uint64_t ex, tot;
    block_scan<1, kT>(&done, &ex, &tot);
    if (threadIdx.x == 0) a.part_r[(uint64_t)blockIdx.x * 8 + kCbcsRBlocks] = tot;
}

__global__ __launch_bounds__(kPlanLanes) void k_cbcs_summary(CencArgs a)
{
    if (a.ctl[kCencCErr] != 0) return;
    uint64_t v = 0, ex, tot;
    for (uint32_t g = threadIdx.x; g < kCencRanges; g += kPlanLanes) v += a.part_r[(uint64_t)g * 8 + kCbcsRBlocks];
    block_scan<1, kPlanLanes>(&v, &ex, &tot);
    if (threadIdx.x == 0) a.summary->rbsp_bytes = 16u * tot;
}

} // namespace

hipError_t launch_cbcs_crypt(const CbcsCall& c, hipStream_t st)
{
    const CencArgs& a = c;
    const hipError_t e = begin_launches(a.ev_begin, st);
    if (e != hipSuccess) return e;
    enqueue_cenc_checks(a, st);
    if (a.n_samples) {
        CbcsKernelArgs k;
        k.pattern = c.pattern;
        for (int i = 0; i < 4; ++i) k.iv0[i] = c.iv0[i];
        if (c.decrypt) hipLaunchKernelGGL((k_cbcs_crypt<true>), dim3(kCencRanges), dim3(kT), 0, st, a, k, c.dk);
        else hipLaunchKernelGGL((k_cbcs_crypt<false>), dim3(kCencRanges), dim3(kT), 0, st, a, k, c.ek);
        hipLaunchKernelGGL(k_cbcs_summary, dim3(1), dim3(kPlanLanes), 0, st, a);
    }
    return end_launches(a.ev_end, st);
}

} // namespace hbs
