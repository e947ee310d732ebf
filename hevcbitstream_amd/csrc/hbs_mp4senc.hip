/*
 * hbs_mp4senc.hip -- hbs_mp4_senc_samples: the senc boxes of protected fMP4 fragments in device memory -> the subsample table
 * and the IVs that hbs_cenc_crypt and hbs_cbcs_crypt read (include/hevcbitstream_amd.h; the rules are mp4senc_find,
 * mp4senc_hint_ok, mp4senc_record and mp4senc_entry, hbs_mp4senc.h).  A senc is a chain of records of variable length, so a
 * sample's place is known only behind the one in front of it; the traf's saiz proposes every place at once, and a proposal is
 * checked against the senc itself.  Thirteen launches, none of which waits for another workgroup, none reads an mdat byte:
 *
 *   k_senc_frag<0>  FIND, a lane a fragment, 256 a workgroup: bounds, the moof's children, the traf mp4rd_moof would read, its
 *                   senc (header checked) and its saiz (kept only when it counts the fragment's samples); per workgroup the
 *                   sums of samples and of fragments with a senc, and 1 + its lowest fragment that is refused
 *   k_senc_scan1    one workgroup: exclusive scan of those sums (scan_parts: hbs_plan.h)
 *   k_senc_frag<1>  the fragments once more, with the sums in front: the numbering rule, each fragment's first sample
 *   k_senc_scan2    one workgroup: the lowest fragment that offends so far, by form or by number; behind one nothing more runs
 *   k_senc_samp<0>  a lane a sample: its fragment by binary search among the first samples, the size saiz gives its record;
 *                   the sums of those that restart at every fragment (block_seg_excl), per workgroup the open sum
 *   k_senc_scan3    one workgroup: the segmented scan of the open sums (seg_scan_parts)
 *   k_senc_samp<1>  COUNT, HINTED: the sample's proposed place is its fragment's first record + the sizes in front; the lane
 *                   reads subsample_count there and accepts the place when IV + 2 + 6 n is the proposed size and the record
 *                   stays in the box (mp4senc_hint_ok), else it marks its fragment.  A sample of a senc without subsample
 *                   tables, or of a traf without a senc, gets its count in closed form from d_sample_size
 *   k_senc_walk     COUNT, SERIAL, a lane a fragment: only the fragments without a usable saiz or with a mark are walked
 *                   record by record (a step a sample, never a byte); the one place a sample can leave its box.  When a fragment
 *                   offends already, those below it are all walked, and nothing is kept: the lowest offender is named
 *   k_senc_sum      a lane a sample: per workgroup the entries
 *   k_senc_verdict  one workgroup: the scan of those, the total, every error but nothing of the summary yet
 *   k_senc_place    a lane a sample: the entries in front of it into the scratch and d_sub_first, its IV as one 16-byte store
 *   k_senc_entries  a lane an ENTRY, min(2 048, 4 per 256 samples) workgroups that stride: its sample by binary search among
 *                   the entries in front, six bytes put together from big-endian words and stored as eight; per workgroup
 *                   the sum of protect (a plan needs it too: rbsp_bytes)
 *   k_senc_finish   one workgroup: the sum of those, the summary
 *
 * Traffic: the box headers of every moof once, saiz once or twice, a 16-bit count a sample, the entries once; 52 bytes a
 * fragment and 16 a sample of scratch.
 */
#include <hip/hip_runtime.h>
#include "hbs_mp4senc.h"
#include "hbs_plan.h"
#include "hbs_copy16.h"

namespace hbs {
namespace {

constexpr int kST = kSencLanes;
static_assert(kSencLanes == kPlanLanes, "the plan's workgroups share block_scan's instances with scan_parts");

/* ctl words: no output is stored; nothing is counted either (HBS_E_ARG, or 2^48 entries); the code; the entries; 1 + the bad
 * fragment, the bad sample; the fragments whose senc was read */
enum : int { kErr = 0, kSkip = 1, kCode = 2, kTotal = 3, kBadFrag = 4, kBadSamp = 5, kSencRead = 6 };

/* ---- fragments --------------------------------------------------------------------------------------------------------- */

/* MODE 0 find, 1 number */
template <int MODE>
__global__ __launch_bounds__(kST) void k_senc_frag(Mp4SencArgs a)
{
    const uint64_t r = (uint64_t)blockIdx.x * kST + threadIdx.x;
    const bool in = r < a.n_frags;
    hbs_mp4_frag f;
    f.out_off = 0; f.out_bytes = 0; f.first_au = 0; f.decode_time = 0; f.samples = 0; f.sequence = 0; f.flags = 0; f.reserved = 0;
    if (in) f = a.frag[r];
    if (MODE == 0) {
        uint64_t bad = 0, v[2] = {f.samples, 0};
        if (in) {
            SencFind o;
            if (!mp4senc_find(a.src, a.n, f, a.track_id, a.V, a.sample_size != nullptr, (a.flags & HBS_SENC_CLEAR_IF_ABSENT) != 0u, o)) {
                bad = r + 1; o.mode = kSencNone;
            }
            v[1] = (o.mode == kSencSub || o.mode == kSencFlatMode) ? 1u : 0u;
            a.find[r] = o;
            a.frag_fail[r] = 0;
        }
        bad = block_min_nonzero(bad);
        uint64_t ex[2], tot[2];
        block_scan<2, kST>(v, ex, tot);
        if (threadIdx.x == 0) {
            unsigned long long* p = a.part_f + (uint64_t)blockIdx.x * 8;
            p[0] = tot[0]; p[1] = tot[1]; p[2] = bad;
        }
        return;
    }
    const uint64_t v = f.samples;
    uint64_t ex, tot;
    block_scan<1, kST>(&v, &ex, &tot);
    uint64_t bad = 0;
    if (in) {
        const uint64_t below = a.part_f[(uint64_t)blockIdx.x * 8] + ex;
        const bool last = r + 1 == a.n_frags;
        if (!mp4prot_numbering_ok(f.first_au - a.frag[0].first_au, below, f.samples, a.n_samples, last)) bad = r + 1;
        a.frag_first[r] = below;
        if (last) a.frag_first[r + 1] = a.n_samples;
    }
    bad = block_min_nonzero(bad);
    if (threadIdx.x == 0) a.bad_num[blockIdx.x] = bad;
}

__global__ __launch_bounds__(kPlanLanes) void k_senc_scan1(Mp4SencArgs a, uint64_t frag_blocks)
{
    uint64_t carry[2];
    const uint64_t bad = scan_parts<2>(a.part_f, frag_blocks, carry);
    if (threadIdx.x == 0) { a.ctl[kBadFrag] = bad; a.ctl[kSencRead] = carry[1]; }
}

__global__ __launch_bounds__(kPlanLanes) void k_senc_scan2(Mp4SencArgs a, uint64_t frag_blocks)
{
    const uint64_t bad_num = min_nonzero_of(a.bad_num, frag_blocks);
    if (threadIdx.x == 0) {
        const uint64_t bad_form = a.ctl[kBadFrag];
        a.ctl[kBadFrag] = bad_form && (!bad_num || bad_form < bad_num) ? bad_form : bad_num;
    }
}

/* ---- samples ----------------------------------------------------------------------------------------------------------- */

/* MODE 0 the hint's open sums, 1 count */
template <int MODE>
__global__ __launch_bounds__(kST) void k_senc_samp(Mp4SencArgs a)
{
    if (a.ctl[kBadFrag] != 0) return;                  /* (the first samples mean nothing then) */
    const uint64_t s = (uint64_t)blockIdx.x * kST + threadIdx.x;
    const bool in = s < a.n_samples;
    uint64_t h = 0, r = 0, i = 0;
    bool head = false;
    SencFind o;
    o.data = 0; o.end = 0; o.saiz_at = 0; o.mode = kSencNone; o.hint = kSencNoHint; o.def = 0; o.pad = 0;
    if (in) {
        r = last_le((uint64_t)0, a.n_frags - 1, s, [&](uint64_t k) { return (uint64_t)a.frag_first[k]; });
        i = s - a.frag_first[r];                       /* (below the fragment's samples: the numbering holds) */
        o = a.find[r];
        head = i == 0;
        if (o.mode == kSencSub && o.hint != kSencNoHint) h = o.hint == kSencHintDefault ? o.def : a.src[o.saiz_at + i];
    }
    uint64_t ex, tot;
    bool exf, totf;
    block_seg_excl<1, kST>(&h, &head, &ex, &exf, &tot, &totf);
    unsigned long long* part = a.part_k + (uint64_t)blockIdx.x * 8;
    if (MODE == 0) {
        if (threadIdx.x == 0) { part[0] = tot; part[1] = totf ? 1 : 0; }
        return;
    }
    uint64_t bad = 0;
    if (in) {
        const uint64_t before = head ? 0 : exf ? ex : ex + part[0];
        uint64_t cnt = 0, rec = 0;
        if (o.mode == kSencSub) {
            if (o.hint != kSencNoHint) {
                uint32_t n;
                if (mp4senc_hint_ok(a.src, o.data, o.end, a.V, before, (uint32_t)h, n)) { cnt = n; rec = o.data + before; }
                else a.frag_fail[r] = 1;
            }
        } else {
            const uint64_t z = a.sample_size[s];       /* (find refused the fragment without a d_sample_size) */
            if (z > 0xFFFFFFFFull) bad = s + 1;
            else if (o.mode == kSencFlatMode) { cnt = mp4senc_flat_count(z); rec = (o.data + (uint64_t)a.V * i) | kSencFlat; }
            else { cnt = mp4senc_clear_count(z); rec = kSencAbsent; }
        }
        a.rec_at[s] = rec; a.first[s] = cnt;
    }
    bad = block_min_nonzero(bad);
    if (threadIdx.x == 0) a.part_c[(uint64_t)blockIdx.x * 8 + 1] = bad;
}

__global__ __launch_bounds__(kPlanLanes) void k_senc_scan3(Mp4SencArgs a, uint64_t samp_blocks)
{
    if (a.ctl[kBadFrag] != 0) return;
    seg_scan_parts<1>(a.part_k, samp_blocks);
}

__global__ __launch_bounds__(kST) void k_senc_walk(Mp4SencArgs a)
{
    /* a fragment offends already: the sample kernels did not run and the first samples may mean nothing.  The fragments below
     * it are all walked, for a lower one whose senc a sample leaves, and nothing is kept */
    const uint64_t stop = a.ctl[kBadFrag];
    const uint64_t r = (uint64_t)blockIdx.x * kST + threadIdx.x;
    uint64_t bad = 0;
    if (r < a.n_frags && (!stop || r + 1 < stop)) {
        const SencFind o = a.find[r];
        if (o.mode == kSencSub && (stop || o.hint == kSencNoHint || a.frag_fail[r] != 0)) {
            const uint64_t s0 = stop ? 0 : a.frag_first[r], S = a.frag[r].samples;
            uint64_t at = o.data;
            for (uint64_t i = 0; i < S; ++i) {
                uint32_t n;
                uint64_t next;
                if (!mp4senc_record(a.src, at, o.end, a.V, n, next)) { bad = r + 1; break; }
                if (!stop) { a.rec_at[s0 + i] = at; a.first[s0 + i] = n; }
                at = next;
            }
        }
    }
    bad = block_min_nonzero(bad);
    if (threadIdx.x == 0) a.bad_walk[blockIdx.x] = bad;
}

__global__ __launch_bounds__(kST) void k_senc_sum(Mp4SencArgs a)
{
    if (a.ctl[kBadFrag] != 0) return;
    const uint64_t s = (uint64_t)blockIdx.x * kST + threadIdx.x;
    const uint64_t c = s < a.n_samples ? a.first[s] : 0;
    uint64_t ex, tot;
    block_scan<1, kST>(&c, &ex, &tot);
    if (threadIdx.x == 0) a.part_c[(uint64_t)blockIdx.x * 8] = tot;
}

__global__ __launch_bounds__(kPlanLanes) void k_senc_verdict(Mp4SencArgs a, uint64_t frag_blocks, uint64_t samp_blocks)
{
    uint64_t bad_frag = a.ctl[kBadFrag], bad_samp = 0, carry[1] = {0};
    const uint64_t bad_walk = min_nonzero_of(a.bad_walk, frag_blocks);        /* (below bad_frag, when both are set) */
    if (!bad_frag) bad_samp = scan_parts<1>(a.part_c, samp_blocks, carry);
    if (bad_walk) bad_frag = bad_walk;
    if (threadIdx.x == 0) {
        const uint64_t total = carry[0];
        int32_t err = 0;
        bool skip = false;
        if (bad_frag) { err = HBS_E_ARG; bad_samp = 0; skip = true; }
        else if (bad_samp) { err = HBS_E_ARG; skip = true; }
        else if (total >= kSencSubLimit) { err = HBS_E_CAPACITY; skip = true; }
        else if (a.sub && total > a.sub_cap) err = HBS_E_CAPACITY;
        a.ctl[kErr] = err ? 1 : 0; a.ctl[kSkip] = skip ? 1 : 0; a.ctl[kCode] = (unsigned long long)(uint32_t)err;
        a.ctl[kTotal] = skip ? 0 : total; a.ctl[kBadFrag] = bad_frag; a.ctl[kBadSamp] = bad_samp;
        if (!err) a.sub_first[a.n_samples] = total;
    }
}

__global__ __launch_bounds__(kST) void k_senc_place(Mp4SencArgs a)
{
    if (a.ctl[kSkip] != 0) return;
    const uint64_t s = (uint64_t)blockIdx.x * kST + threadIdx.x;
    const bool in = s < a.n_samples;
    const uint64_t c = in ? a.first[s] : 0;
    uint64_t ex, tot;
    block_scan<1, kST>(&c, &ex, &tot);
    if (!in) return;
    const uint64_t at = a.part_c[(uint64_t)blockIdx.x * 8] + ex;
    a.first[s] = at;
    if (s + 1 == a.n_samples) a.first[s + 1] = at + c;
    if (a.ctl[kErr] != 0) return;
    a.sub_first[s] = at;
    if (a.V) {
        const uint64_t rec = a.rec_at[s];
        uint32_t w[4] = {0, 0, 0, 0};
        if (!(rec & kSencAbsent)) mp4senc_iv_words(a.src, rec & kSencAtMask, a.V, w);
        *reinterpret_cast<uint4*>(a.iv + 16u * s) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

/* ---- entries ----------------------------------------------------------------------------------------------------------- */

__global__ __launch_bounds__(kST) void k_senc_entries(Mp4SencArgs a)
{
    if (a.ctl[kSkip] != 0) return;
    const uint64_t total = a.ctl[kTotal];
    const bool store = a.sub && a.ctl[kErr] == 0;
    uint64_t sum = 0;
    for (uint64_t e = (uint64_t)blockIdx.x * kST + threadIdx.x; e < total; e += (uint64_t)gridDim.x * kST) {
        /* the last sample whose entries begin at or in front of e: the one that has it (those without entries share a word
         * with the sample behind them) */
        const uint64_t s = last_le((uint64_t)0, a.n_samples - 1, e, [&](uint64_t k) { return (uint64_t)a.first[k]; });
        const uint64_t j = e - a.first[s], rec = a.rec_at[s];
        hbs_cenc_subsample x;
        if (rec & kSencFlat) { x.clear = 0; x.protect = (uint32_t)a.sample_size[s]; }
        else if (rec & kSencAbsent) x = mp4senc_clear_entry(a.sample_size[s], j);
        else x = mp4senc_entry(a.src, rec, a.V, j);
        sum += x.protect;
        if (store) *reinterpret_cast<uint2*>(a.sub + e) = make_uint2(x.clear, x.protect);
    }
    uint64_t ex, tot;
    block_scan<1, kST>(&sum, &ex, &tot);
    if (threadIdx.x == 0) a.part_p[(uint64_t)blockIdx.x * 8] = tot;
}

__global__ __launch_bounds__(kPlanLanes) void k_senc_finish(Mp4SencArgs a, uint64_t ent_blocks)
{
    const bool skip = a.ctl[kSkip] != 0;
    uint64_t sum = 0;
    if (!skip) for (uint64_t i = threadIdx.x; i < ent_blocks; i += kPlanLanes) sum += a.part_p[i * 8];
    uint64_t ex, tot;
    block_scan<1, kPlanLanes>(&sum, &ex, &tot);
    if (threadIdx.x == 0) {
        hbs_summary s;
        s.nal_count = a.ctl[kTotal]; s.nal_found = a.n_samples; s.rbsp_bytes = skip ? 0 : tot; s.stream_bytes = a.n; s.stop_reason = 0;
        s.error = (int32_t)(uint32_t)a.ctl[kCode];
        s.reserved[0] = a.ctl[kBadSamp]; s.reserved[1] = a.ctl[kBadFrag]; s.reserved[2] = skip ? 0 : a.ctl[kSencRead];
        *a.summary = s;
    }
}

} // namespace

hipError_t launch_mp4_senc_samples(const Mp4SencArgs& a, hipStream_t st)
{
    const uint64_t fb = (a.n_frags + kST - 1) / kST, sb = (a.n_samples + kST - 1) / kST, eb = a.ent_blocks;
    const hipError_t e = begin_launches(a.ev_begin, st);
    if (e != hipSuccess) return e;
    if (fb) hipLaunchKernelGGL(k_senc_frag<0>, dim3((unsigned)fb), dim3(kST), 0, st, a);
    hipLaunchKernelGGL(k_senc_scan1, dim3(1), dim3(kPlanLanes), 0, st, a, fb);
    if (fb) hipLaunchKernelGGL(k_senc_frag<1>, dim3((unsigned)fb), dim3(kST), 0, st, a);
    hipLaunchKernelGGL(k_senc_scan2, dim3(1), dim3(kPlanLanes), 0, st, a, fb);
    if (sb) {
        hipLaunchKernelGGL(k_senc_samp<0>, dim3((unsigned)sb), dim3(kST), 0, st, a);
        hipLaunchKernelGGL(k_senc_scan3, dim3(1), dim3(kPlanLanes), 0, st, a, sb);
        hipLaunchKernelGGL(k_senc_samp<1>, dim3((unsigned)sb), dim3(kST), 0, st, a);
        hipLaunchKernelGGL(k_senc_walk, dim3((unsigned)fb), dim3(kST), 0, st, a);
        hipLaunchKernelGGL(k_senc_sum, dim3((unsigned)sb), dim3(kST), 0, st, a);
    }
    hipLaunchKernelGGL(k_senc_verdict, dim3(1), dim3(kPlanLanes), 0, st, a, sb ? fb : 0, sb);
    if (sb) {
        hipLaunchKernelGGL(k_senc_place, dim3((unsigned)sb), dim3(kST), 0, st, a);
        hipLaunchKernelGGL(k_senc_entries, dim3((unsigned)eb), dim3(kST), 0, st, a);
    }
    hipLaunchKernelGGL(k_senc_finish, dim3(1), dim3(kPlanLanes), 0, st, a, sb ? eb : 0);
    return end_launches(a.ev_end, st);
}

} // namespace hbs

extern "C" {

int64_t hbs_mp4_init_unprotect_host(const uint8_t* init, uint64_t n, uint32_t track_id, hbs_mp4_tenc* t_out, uint32_t* format_out,
                                    uint64_t* pssh_off, uint64_t* pssh_bytes, uint64_t pssh_cap, uint64_t* n_pssh_out, uint8_t* out, uint64_t cap)
{
    return hbs::mp4_init_unprotect(init, n, track_id, t_out, format_out, pssh_off, pssh_bytes, pssh_cap, n_pssh_out, out, cap);
}

}
