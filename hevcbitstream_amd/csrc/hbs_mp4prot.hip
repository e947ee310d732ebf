/*
 * hbs_mp4prot.hip -- hbs_mp4_protect: the fragments hbs_mp4_fragment wrote -> the same fragments with saiz, saio and senc in
 * every traf, back to back (include/hevcbitstream_amd.h; the rules are mp4prot_frag_ok, mp4prot_sample_tables,
 * mp4prot_sample_entries and mp4prot_moof_byte, hbs_mp4prot.h).  A plan over the fragments and one over the samples, then a copy
 * over 64 KiB output tiles.  Eleven launches, none of which waits for another workgroup:
 *
 *   k_prot_frag<0>  a lane a fragment, 256 a workgroup: the fragment rule on its header words; per workgroup the sums of
 *                   samples and bytes and 1 + its lowest fragment that is not in the form
 *   k_prot_samp<0>  a lane a sample: the first group of the sample rule (d_sub_first, the entry count, the IV's tail), which
 *                   reads no entry; per workgroup 1 + its lowest offender
 *   k_prot_scan     one workgroup: exclusive scan of the fragments' sums (scan_parts: hbs_plan.h); what was wrong so far
 *   k_prot_frag<1>  the fragments once more, with the sums in front: the numbering rule; E_r = the d_sub_first words at its two
 *                   ends, so where the fragment, its mdat and its source bytes lie follows in closed form (the entries below
 *                   fragment r are d_sub_first[its first sample]); whether its new moof is too large
 *   k_prot_scan2    one workgroup: the lowest fragment that offends, by form or by number
 *   k_prot_samp<1>  only when no fragment offends and the first group holds everywhere: a lane a sample, its fragment by binary
 *                   search among the first samples, the size word of its trun entry, its entries (42 at most) added up; the
 *                   sizes' sums that restart at every fragment (block_seg_excl)
 *   k_prot_finish   one workgroup: the segmented scan of those over the workgroups, the error, the totals, the summary.  A
 *                   plan-only call ends here
 *   k_prot_frag<2>  d_frag_out;  k_prot_samp<2>  d_sample_off / d_sample_size (each only when asked for)
 *   k_prot_tiles    a lane per 64 KiB output tile: binary search of the fragment its first byte lies in
 *   k_prot_copy     one workgroup per output tile: the tile's fragments (at most 442: a fragment has 149 bytes or more) are
 *                   staged in LDS; each lane takes 16-byte output chunks 4 KiB apart, in the skeleton of hbs_copy16.h:
 *                   copy_batches for the chunks wholly inside one fragment's mdat (header and payload, which come from the
 *                   source at any byte offset); the chunks that hold moof bytes or span two fragments go to the list in LDS,
 *                   and copy_slow_list makes their bytes through mp4prot_moof_byte (chunk_byte).
 *
 * Traffic: the mdats read once and the output written once; thirteen header words a fragment, the fragment table three times,
 * d_sub_first by each sample pass, the entries twice (the sums, the senc), the trun size words twice; 32 B a fragment and 8 B a
 * tile of scratch.
 */
#include <hip/hip_runtime.h>
#include "hbs_mp4prot.h"
#include "hbs_plan.h"
#include "hbs_copy16.h"

namespace hbs {
namespace {

constexpr int kPT = kProtLanes;
constexpr uint32_t kTile = (uint32_t)kProtTileBytes;
constexpr int kChunks = (int)(kProtTileBytes / 16 / kPT);             /* 16-byte output chunks a copy lane takes  */
constexpr uint32_t kMinFrag = kMp4FragFixed + kProtFixed;             /* a protected fragment of no samples and an empty mdat */
constexpr uint32_t kLdsFrags = 448;                                   /* fragments a tile can hold, and two       */
static_assert(kProtTileBytes / kMinFrag + 3 <= kLdsFrags, "every fragment of a tile is staged");
static_assert(kProtLanes == kPlanLanes, "the plan's workgroups share block_scan's instances with scan_parts");

enum : int { kErr = 0, kTotal = 1, kBadFrag = 2, kBadTab = 3, kInBytes = 4, kTooLarge = 5, kBig = 6 };      /* ctl words */

/* ---- fragments --------------------------------------------------------------------------------------------------------- */

/* MODE 0 count, 1 place, 2 d_frag_out */
template <int MODE>
__global__ __launch_bounds__(kPT) void k_prot_frag(Mp4ProtArgs a)
{
    if (MODE == 2 && a.ctl[kErr] != 0) return;
    const uint64_t r = (uint64_t)blockIdx.x * kPT + threadIdx.x;
    const bool in = r < a.n_frags;
    hbs_mp4_frag f;
    f.out_off = 0; f.out_bytes = 0; f.first_au = 0; f.decode_time = 0; f.samples = 0; f.sequence = 0; f.flags = 0; f.reserved = 0;
    if (in) f = a.frag[r];
    if (MODE == 2) {
        if (!in) return;
        f.out_off = a.frag_at[r]; f.out_bytes = a.frag_at[r + 1] - a.frag_at[r];
        a.frag_out[r] = f;
        return;
    }
    if (MODE == 0) {
        uint64_t bad = 0;
        if (in && !mp4prot_frag_ok(a.src, a.n, f)) { bad = r + 1; f.out_bytes = 0; }
        const uint64_t v[3] = {f.samples, f.out_bytes, f.out_bytes >> 20};
        bad = block_min_nonzero(bad);
        uint64_t ex[3], tot[3];
        block_scan<3, kPT>(v, ex, tot);
        if (threadIdx.x == 0) {
            unsigned long long* p = a.part_f + (uint64_t)blockIdx.x * 8;
            p[0] = tot[0]; p[1] = tot[1]; p[2] = tot[2]; p[3] = bad;
        }
        return;
    }
    /* (with a fragment that is not in the form the bytes' sums mean nothing, and nothing is made of them) */
    const uint64_t v[2] = {f.samples, f.out_bytes};
    uint64_t ex[2], tot[2];
    block_scan<2, kPT>(v, ex, tot);
    uint64_t bad = 0, big = 0;
    if (in) {
        const unsigned long long* p = a.part_f + (uint64_t)blockIdx.x * 8;
        const uint64_t below = p[0] + ex[0], bytes_below = p[1] + ex[1], S = f.samples, N = a.n_samples;
        const bool last = r + 1 == a.n_frags;
        if (!mp4prot_numbering_ok(f.first_au - a.frag[0].first_au, below, S, N, last)) bad = r + 1;
        else {
            /* (d_sub_first is read whatever it holds: below + S <= n_samples; what a wrong one makes of these is not used) */
            const uint64_t e0 = N ? a.sub_first[below] : 0, E = S ? a.sub_first[below + S] - e0 : 0;
            const uint64_t moof = mp4prot_moof_bytes(S, E, a.V);
            if (moof > kProtMoofMax) big = r + 1;              /* (reported only when the samples hold: E is 42 S at most then) */
            const uint64_t at = bytes_below + (uint64_t)kProtFixed * r + (a.V + 3ull) * below + 6u * e0;
            a.frag_first[r] = below; a.frag_at[r] = at; a.frag_body[r] = at + moof;
            a.frag_delta[r] = f.out_off + kMp4MoofHead + 16u * S - (at + moof);
            if (last) { a.frag_first[r + 1] = N; a.frag_at[r + 1] = at + f.out_bytes + mp4prot_growth(S, E, a.V); }
        }
    }
    bad = block_min_nonzero(bad);
    big = block_min_nonzero(big);
    if (threadIdx.x == 0) { a.bad_num[blockIdx.x] = bad; a.bad_big[blockIdx.x] = big; }
}

__global__ __launch_bounds__(kPlanLanes) void k_prot_scan(Mp4ProtArgs a, uint64_t frag_blocks, uint64_t samp_blocks)
{
    uint64_t carry[3];
    const uint64_t bad_form = scan_parts<3>(a.part_f, frag_blocks, carry);
    const uint64_t bad_tab = min_nonzero_of(a.bad_tab, samp_blocks);
    if (threadIdx.x == 0) {
        a.ctl[kBadFrag] = bad_form; a.ctl[kBadTab] = bad_tab; a.ctl[kInBytes] = carry[1];
        a.ctl[kTooLarge] = carry[2] + a.n_frags >= kProtBytesLimit ? 1 : 0;
    }
}

__global__ __launch_bounds__(kPlanLanes) void k_prot_scan2(Mp4ProtArgs a, uint64_t frag_blocks)
{
    const uint64_t bad_num = min_nonzero_of(a.bad_num, frag_blocks);
    const uint64_t big = min_nonzero_of(a.bad_big, frag_blocks);
    if (threadIdx.x == 0) {
        const uint64_t bad_form = a.ctl[kBadFrag];
        a.ctl[kBadFrag] = bad_form && (!bad_num || bad_form < bad_num) ? bad_form : bad_num;
        a.ctl[kBig] = big;
    }
}

/* ---- samples ----------------------------------------------------------------------------------------------------------- */

/* MODE 0 the first group, 1 the second and the sizes' sums, 2 the sample tables */
template <int MODE>
__global__ __launch_bounds__(kPT) void k_prot_samp(Mp4ProtArgs a)
{
    const uint64_t s = (uint64_t)blockIdx.x * kPT + threadIdx.x;
    const bool in = s < a.n_samples;
    if (MODE == 0) {
        const bool ok = !in || mp4prot_sample_tables(reinterpret_cast<const uint64_t*>(a.sub_first), a.iv, a.V, s);
        const uint64_t bad = block_min_nonzero(ok ? 0 : s + 1);
        if (threadIdx.x == 0) a.bad_tab[blockIdx.x] = bad;
        return;
    }
    if (MODE == 1 ? (a.ctl[kBadFrag] != 0 || a.ctl[kBadTab] != 0) : a.ctl[kErr] != 0) return;
    uint64_t size = 0, r = 0;
    bool head = false;
    if (in) {
        r = last_le((uint64_t)0, a.n_frags - 1, s, [&](uint64_t i) { return (uint64_t)a.frag_first[i]; });
        const uint64_t i = s - a.frag_first[r];
        size = rd_be32(a.src, a.frag[r].out_off + kMp4MoofHead + 16u * i + 4u);
        head = i == 0;
    }
    uint64_t ex, tot;
    bool exf, totf;
    block_seg_excl<1, kPT>(&size, &head, &ex, &exf, &tot, &totf);
    unsigned long long* part = a.part_k + (uint64_t)blockIdx.x * 8;
    if (MODE == 1) {
        bool ok = true;
        if (in) {
            const uint64_t first = a.sub_first[s];
            ok = mp4prot_sample_entries(a.sub, first, (uint32_t)(a.sub_first[s + 1] - first), (uint32_t)size);
        }
        const uint64_t bad = block_min_nonzero(ok ? 0 : s + 1);
        if (threadIdx.x == 0) { part[0] = tot; part[1] = totf ? 1 : 0; a.bad_ent[blockIdx.x] = bad; }
        return;
    }
    if (!in) return;
    const uint64_t before = head ? 0 : exf ? ex : ex + part[0];
    a.sample_off[s] = a.frag_body[r] + 8u + before;
    a.sample_size[s] = size;
}

__global__ __launch_bounds__(kPlanLanes) void k_prot_finish(Mp4ProtArgs a, uint64_t samp_blocks)
{
    const uint64_t bad_frag = a.ctl[kBadFrag], bad_tab = a.ctl[kBadTab];
    uint64_t bad_ent = 0;
    if (!bad_frag && !bad_tab) {                             /* (else the entries were not looked at) */
        bad_ent = min_nonzero_of(a.bad_ent, samp_blocks);
        seg_scan_parts<1>(a.part_k, samp_blocks);
    }
    if (threadIdx.x == 0) {
        const uint64_t R = a.n_frags, N = a.n_samples, E = N ? a.sub_first[N] : 0, big = a.ctl[kBig];
        const uint64_t total = a.ctl[kInBytes] + (uint64_t)kProtFixed * R + (a.V + 3ull) * N + 6u * E;
        hbs_summary s;
        s.nal_count = R; s.nal_found = N; s.rbsp_bytes = 0; s.stream_bytes = 0; s.stop_reason = 0;
        s.reserved[0] = 0; s.reserved[1] = 0; s.reserved[2] = 0;
        int32_t err = 0;
        if (bad_frag) { err = HBS_E_ARG; s.reserved[1] = bad_frag; }
        else if (bad_tab || bad_ent) { err = HBS_E_ARG; s.reserved[0] = bad_tab ? bad_tab : bad_ent; }
        else if (big) { err = HBS_E_ARG; s.reserved[1] = big; }
        else if (a.ctl[kTooLarge]) err = HBS_E_CAPACITY;
        else {
            s.rbsp_bytes = E; s.stream_bytes = total;
            if (a.out && total > a.out_cap) err = HBS_E_CAPACITY;
        }
        s.error = err;
        a.ctl[kErr] = err ? 1 : 0; a.ctl[kTotal] = total;
        *a.summary = s;
    }
}

/* ---- the copy ---------------------------------------------------------------------------------------------------------- */

__global__ __launch_bounds__(256) void k_prot_tiles(Mp4ProtArgs a)
{
    if (a.ctl[kErr] != 0) return;
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t > a.tiles) return;
    tile_first_of<kTile>(a.frag_at, a.n_frags, a.ctl[kTotal], t, a.tile_frag);
}

/* the tile's fragments [r0, r0 + fcnt), staged in LDS */
struct TileFrags {
    const unsigned long long* s_at; const unsigned long long* s_body; const unsigned long long* s_delta;
    uint64_t r0;
    uint32_t fcnt;
    __device__ __forceinline__ uint64_t at(uint32_t i) const { return s_at[i]; }                       /* i = fcnt: the end */
    __device__ __forceinline__ uint32_t find(uint32_t lo, uint64_t o) const
    {
        return last_le(lo, fcnt - 1, o, [&](uint32_t i) { return at(i); });
    }
};

/* output byte `cur` of a chunk that holds moof bytes or spans fragments (or ends the output), from the rule; fi: the fragment
 * the chunk's first byte lies in (a fragment has 149 bytes or more: the byte lies in it or in the next) */
__device__ __forceinline__ uint32_t chunk_byte(const Mp4ProtArgs& a, const TileFrags& tf, uint32_t fi, uint64_t cur)
{
    fi += cur >= tf.at(fi + 1) ? 1u : 0u;
    if (cur >= tf.s_body[fi]) return a.src[cur + tf.s_delta[fi]];
    const uint64_t r = tf.r0 + fi, first = a.frag_first[r];
    const uint32_t S = a.frag[r].samples;
    const uint64_t* sf = reinterpret_cast<const uint64_t*>(a.sub_first) + first;
    const uint64_t E = S ? sf[S] - sf[0] : 0;
    return mp4prot_moof_byte(a.src, a.frag[r].out_off, S, E, a.V, sf, a.sub, a.iv + 16u * first, cur - tf.at(fi));
}

__global__ __launch_bounds__(kPT) void k_prot_copy(Mp4ProtArgs a)
{
    __shared__ unsigned long long s_at[kLdsFrags + 1];
    __shared__ unsigned long long s_body[kLdsFrags];
    __shared__ unsigned long long s_delta[kLdsFrags];
    __shared__ uint32_t s_slow[kTile / 16];           /* the chunks done byte by byte: chunk | its fragment's number in the tile << 12 */
    __shared__ uint32_t s_nslow;
    if (a.ctl[kErr] != 0) return;
    const uint64_t total = a.ctl[kTotal];
    const uint64_t t0 = (uint64_t)blockIdx.x * kTile;
    if (t0 >= total) return;
    const uint32_t tlen = total - t0 < kTile ? (uint32_t)(total - t0) : kTile;
    const uint64_t r0 = a.tile_frag[blockIdx.x], r1 = a.tile_frag[blockIdx.x + 1];
    const uint64_t fwant = r1 - r0 + 1;               /* fragments [r0, r1]; frag_at[r1 + 1] exists (the total at the end) */
    TileFrags tf;
    tf.s_at = s_at; tf.s_body = s_body; tf.s_delta = s_delta; tf.r0 = r0;
    tf.fcnt = fwant < kLdsFrags ? (uint32_t)fwant : kLdsFrags;            /* (never more: the static_assert above) */
    for (uint32_t i = threadIdx.x; i <= tf.fcnt; i += kPT) {
        s_at[i] = a.frag_at[r0 + i];
        if (i < tf.fcnt) { s_body[i] = a.frag_body[r0 + i]; s_delta[i] = a.frag_delta[r0 + i]; }
    }
    if (threadIdx.x == 0) s_nslow = 0;
    __syncthreads();
    uint32_t flo = 0;
    copy_batches<kPT, kChunks>(a.src, a.out + t0, tlen,
        [&](uint32_t r, uint32_t& fi, uint64_t& s) {
            const uint64_t o = t0 + r;
            fi = flo = tf.find(flo, o);
            /* wholly in the fragment's mdat, header or payload: source bytes */
            if (o < s_body[flo] || o + 16 > tf.at(flo + 1)) return false;
            s = o + s_delta[flo];
            return true;
        },
        [&](uint32_t r, uint32_t fi) { slow_push<kTile>(s_slow, s_nslow, r, fi); });
    __syncthreads();
    copy_slow_list<kPT>(s_slow, s_nslow, a.out, t0, tlen, [&](uint32_t fi, uint64_t cur) { return chunk_byte(a, tf, fi, cur); });
}

} // namespace

hipError_t launch_mp4_protect(const Mp4ProtArgs& a, hipStream_t st)
{
    const uint64_t fb = (a.n_frags + kPT - 1) / kPT, sb = (a.n_samples + kPT - 1) / kPT;
    const hipError_t e = begin_launches(a.ev_begin, st);
    if (e != hipSuccess) return e;
    if (fb) hipLaunchKernelGGL(k_prot_frag<0>, dim3((unsigned)fb), dim3(kPT), 0, st, a);
    if (sb) hipLaunchKernelGGL(k_prot_samp<0>, dim3((unsigned)sb), dim3(kPT), 0, st, a);
    hipLaunchKernelGGL(k_prot_scan, dim3(1), dim3(kPlanLanes), 0, st, a, fb, sb);
    if (fb) hipLaunchKernelGGL(k_prot_frag<1>, dim3((unsigned)fb), dim3(kPT), 0, st, a);
    hipLaunchKernelGGL(k_prot_scan2, dim3(1), dim3(kPlanLanes), 0, st, a, fb);
    if (sb) hipLaunchKernelGGL(k_prot_samp<1>, dim3((unsigned)sb), dim3(kPT), 0, st, a);
    hipLaunchKernelGGL(k_prot_finish, dim3(1), dim3(kPlanLanes), 0, st, a, sb);
    if (a.out && fb) {
        if (a.frag_out) hipLaunchKernelGGL(k_prot_frag<2>, dim3((unsigned)fb), dim3(kPT), 0, st, a);
        if (a.sample_off && sb) hipLaunchKernelGGL(k_prot_samp<2>, dim3((unsigned)sb), dim3(kPT), 0, st, a);
        if (a.tiles) {
            hipLaunchKernelGGL(k_prot_tiles, dim3((unsigned)((a.tiles + 1 + 255) / 256)), dim3(256), 0, st, a);
            hipLaunchKernelGGL(k_prot_copy, dim3((unsigned)a.tiles), dim3(kPT), 0, st, a);
        }
    }
    return end_launches(a.ev_end, st);
}

} // namespace hbs

extern "C" {

uint64_t hbs_mp4_protect_bytes_host(uint64_t samples, uint64_t entries, uint32_t iv_size)
{
    return hbs::mp4prot_growth(samples, entries, iv_size);
}

int64_t hbs_mp4_init_protect_host(const uint8_t* init, uint64_t n, uint32_t track_id, const hbs_mp4_tenc* t,
                                  const uint8_t* const* pssh, const uint64_t* pssh_bytes, uint64_t n_pssh, uint8_t* out, uint64_t cap)
{
    return hbs::mp4_init_protect(init, n, track_id, t, pssh, pssh_bytes, n_pssh, out, cap);
}

}
