/*
 * hbs_lenpref.hip -- hbs_annexb_to_lenpref and hbs_lenpref_to_annexb: Annex-B to length-prefixed NAL units (MP4 / ISOBMFF
 * samples, ISO/IEC 14496-15) and back (include/hevcbitstream_amd.h).  Both are a plan that ends in a table of "pieces" -- a
 * short literal prefix followed by a run of source bytes at its own byte misalignment -- and the copy over that table
 * (hbs_pieces.h).  A plan of three launches and the copy's two each, none of which waits for another workgroup:
 *
 *   k_a2l_count / k_l2a_count   forward: one lane per 8 consecutive NALs checks the entries, the length limit and the AU
 *                    table; reverse: one lane per sample walks its chain of records.  Per workgroup the sums of output bytes
 *                    and records (forward: and kept rbsp_len), and what was wrong
 *   k_a2l_scan / k_l2a_scan     one workgroup: exclusive scan of those sums over the workgroups; totals, the error and the
 *                    summary.  A plan-only call ends here
 *   k_a2l_place / k_l2a_place   the entries / the chains once more, now with the offsets: the piece table, the output index /
 *                    the sample tables
 *   copy_pieces      (hbs_pieces.hip) a lane per 64 KiB output tile finds the piece its first byte lies in, then a workgroup
 *                    per tile copies: the same two kernels as behind the filter's plan
 *
 * Traffic: the payloads read once and written once; forward the index read twice (32 B a NAL) and 32 B a kept NAL of output
 * index, reverse the length fields read twice by the lane of their sample; 16 B a piece of scratch written and read, 8 B a tile.
 */
#include <hip/hip_runtime.h>
#include "hbs_lenpref.h"
#include "hbs_plan.h"

namespace hbs {
namespace {

constexpr int kLT = kPlanLanes;                                       /* lanes of the plan workgroups            */
constexpr int kLPer = kLenprefNalsPerBlock / kLT;                     /* NALs a forward plan lane takes          */
static_assert(kLenprefSamplesPerBlock == kLT, "one lane per sample");

/* ---- Annex-B to length-prefixed ---------------------------------------------------------------------------------------- */

struct Nal {
    uint64_t start, end;
    uint32_t rbsp_len, au;
    int32_t status;
    bool bad, kept, first_of_au;
};

/* entry k with the end of entry k-1 (0 for k = 0) and the AU number of NAL k-1: every check of the call that is about NAL k */
__device__ __forceinline__ Nal eval_nal(const A2lArgs& a, uint64_t k, uint64_t prev_end, uint32_t prev_au)
{
    const hbs_nal_entry e = a.index[k];
    Nal r;
    r.start = e.start; r.end = e.end; r.rbsp_len = e.rbsp_len; r.status = e.status;
    r.bad = e.start > e.end || e.end > a.n || e.start < prev_end;
    r.kept = !r.bad && (!a.keep || a.keep[k] != 0);
    if (r.kept && a.t.prefix < 8 && ((e.end - e.start) >> (8u * a.t.prefix)) != 0) { r.bad = true; r.kept = false; }
    r.au = 0; r.first_of_au = false;
    if (a.nal_au) {
        r.au = a.nal_au[k];
        r.first_of_au = k == 0 || r.au != prev_au;
        if (k == 0 ? r.au != 0 : (r.au != prev_au && (uint64_t)r.au != (uint64_t)prev_au + 1)) r.bad = true;
        if (k == a.n_nals - 1 && (uint64_t)r.au + 1 != a.n_aus) r.bad = true;
    }
    return r;
}

__global__ __launch_bounds__(kLT) void k_a2l_count(A2lArgs a)
{
    const uint64_t base = (uint64_t)blockIdx.x * kLenprefNalsPerBlock + (uint64_t)threadIdx.x * kLPer;
    uint64_t v[3] = {0, 0, 0};
    bool bad = false;
    if (base < a.n_nals) {
        uint64_t prev = base ? a.index[base - 1].end : 0;
        uint32_t pau = (base && a.nal_au) ? a.nal_au[base - 1] : 0;
        for (int i = 0; i < kLPer && base + i < a.n_nals; ++i) {
            const Nal x = eval_nal(a, base + i, prev, pau);
            prev = x.end; pau = x.au;
            bad |= x.bad;
            if (x.kept) { v[0] += a.t.prefix + (x.end - x.start); v[1] += 1; v[2] += x.rbsp_len; }
        }
    }
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    uint64_t ex[3], tot[3];
    block_scan<3, kLT>(v, ex, tot);
    if (threadIdx.x == 0) {
        unsigned long long* p = a.part + (uint64_t)blockIdx.x * 8;
        p[0] = tot[0]; p[1] = tot[1]; p[2] = tot[2]; p[3] = any_bad ? 1 : 0;
    }
}

__global__ __launch_bounds__(kLT) void k_a2l_scan(A2lArgs a, uint64_t blocks)
{
    uint64_t carry[3];
    const uint64_t bad = scan_parts<3>(a.part, blocks, carry) | ((a.nal_au && !a.n_nals && a.n_aus) ? 1 : 0);
    if (threadIdx.x == 0) {
        const uint64_t total = carry[0], kept = carry[1], rbsp = carry[2];
        const int32_t err = bad ? HBS_E_ARG : (a.t.out && total > a.out_cap) ? HBS_E_CAPACITY : 0;
        a.t.ctl[0] = (unsigned long long)(uint32_t)err;
        a.t.ctl[1] = total; a.t.ctl[2] = kept;
        if (!err && a.t.out) {
            a.t.piece_out[kept] = total;
            if (a.nal_au && a.sample_off) a.sample_off[a.n_aus] = total;
        }
        hbs_summary s;
        s.nal_count = kept; s.nal_found = a.n_nals; s.rbsp_bytes = rbsp; s.stream_bytes = total;
        s.stop_reason = 0; s.error = err;
        s.reserved[0] = s.reserved[1] = s.reserved[2] = 0;
        *a.summary = s;
    }
}

__global__ __launch_bounds__(kLT) void k_a2l_place(A2lArgs a)
{
    if (a.t.ctl[0] != 0) return;
    const uint64_t base = (uint64_t)blockIdx.x * kLenprefNalsPerBlock + (uint64_t)threadIdx.x * kLPer;
    const bool in = base < a.n_nals;
    Nal x[kLPer];                       /* the lane's entries, read once: kept in registers across the scan */
    uint64_t v[3] = {0, 0, 0};
    uint64_t prev = (base && in) ? a.index[base - 1].end : 0;
    uint32_t pau = (base && in && a.nal_au) ? a.nal_au[base - 1] : 0;
#pragma unroll
    for (int i = 0; i < kLPer; ++i) {
        x[i].kept = false; x[i].first_of_au = false;
        if (base + i < a.n_nals) {
            x[i] = eval_nal(a, base + i, prev, pau);
            prev = x[i].end; pau = x[i].au;
            if (x[i].kept) { v[0] += a.t.prefix + (x[i].end - x[i].start); v[1] += 1; v[2] += x[i].rbsp_len; }
        }
    }
    uint64_t off[3], tot[3];
    block_scan<3, kLT>(v, off, tot);
    if (!in) return;
    const unsigned long long* p = a.part + (uint64_t)blockIdx.x * 8;
#pragma unroll
    for (int q = 0; q < 3; ++q) off[q] += p[q];
#pragma unroll
    for (int i = 0; i < kLPer; ++i) {
        if (x[i].first_of_au && a.sample_off) a.sample_off[x[i].au] = off[0];
        if (!x[i].kept) continue;
        const uint64_t len = x[i].end - x[i].start, pay = off[0] + a.t.prefix;
        if (a.index_out) {
            hbs_nal_entry o;
            o.start = pay; o.end = pay + len;
            o.rbsp_off = off[2]; o.rbsp_len = x[i].rbsp_len;
            o.status = x[i].status & ~HBS_ST_UNTERMINATED;
            a.index_out[off[1]] = o;
        }
        a.t.piece_out[off[1]] = off[0];
        a.t.piece_delta[off[1]] = x[i].start - pay;
        off[0] = pay + len; off[1] += 1; off[2] += x[i].rbsp_len;
    }
}

/* ---- length-prefixed to Annex-B ---------------------------------------------------------------------------------------- */

/* Sample s, record by record: f(where the payload begins in the input, its length).  recs / pay: the well-formed records in
 * front of the sample's end or of what is wrong with it.  false: the sample leaves the buffer or its chain is malformed.
 * One lane walks one sample: each length field is a load that the next one's address depends on. */
template <class F>
__device__ __forceinline__ bool walk_sample(const L2aArgs& a, uint64_t s, uint64_t& recs, uint64_t& pay, F f)
{
    const uint64_t off = a.sample_off[s], size = a.sample_size[s];
    const uint32_t L = a.length_size;
    recs = 0; pay = 0;
    if (off > a.n || size > a.n - off) return false;
    uint64_t p = off;
    const uint64_t e = off + size;
#pragma unroll 1
    while (p < e) {
        if (e - p < L) return false;
        uint64_t len = 0;
        for (uint32_t b = 0; b < L; ++b) len = (len << 8) | a.t.src[p + b];
        p += L;
        if (len > e - p) return false;
        f(p, len);
        p += len; recs += 1; pay += len;
    }
    return true;
}

__global__ __launch_bounds__(kLT) void k_l2a_count(L2aArgs a)
{
    const uint64_t s = (uint64_t)blockIdx.x * kLT + threadIdx.x;
    uint64_t v[3] = {0, 0, 0};
    uint64_t bad = 0;
    if (s < a.n_samples) {
        uint64_t recs, pay;
        if (!walk_sample(a, s, recs, pay, [](uint64_t, uint64_t) {})) bad = s + 1;
        v[0] = recs * a.t.prefix + pay; v[1] = recs;
        a.samp[2 * s] = v[0]; a.samp[2 * s + 1] = recs;
    }
    bad = block_min_nonzero(bad);
    uint64_t ex[3], tot[3];
    block_scan<3, kLT>(v, ex, tot);
    if (threadIdx.x == 0) {
        unsigned long long* p = a.part + (uint64_t)blockIdx.x * 8;
        p[0] = tot[0]; p[1] = tot[1]; p[2] = 0; p[3] = bad;
    }
}

__global__ __launch_bounds__(kLT) void k_l2a_scan(L2aArgs a, uint64_t blocks)
{
    uint64_t carry[3];
    const uint64_t bad = scan_parts<3>(a.part, blocks, carry);
    if (threadIdx.x == 0) {
        const uint64_t total = carry[0], recs = carry[1];
        const int32_t err = bad ? HBS_E_ARG : (recs > a.nal_cap || (a.t.out && total > a.out_cap)) ? HBS_E_CAPACITY : 0;
        a.t.ctl[0] = (unsigned long long)(uint32_t)err;
        a.t.ctl[1] = total; a.t.ctl[2] = recs;
        if (!err && a.t.out) {
            a.t.piece_out[recs] = total;
            if (a.sample_off_out) a.sample_off_out[a.n_samples] = total;
        }
        hbs_summary s;
        s.nal_count = recs; s.nal_found = a.n_samples; s.rbsp_bytes = 0; s.stream_bytes = total;
        s.stop_reason = recs ? -1 : 0; s.error = err;
        s.reserved[0] = bad; s.reserved[1] = s.reserved[2] = 0;
        *a.summary = s;
    }
}

__global__ __launch_bounds__(kLT) void k_l2a_place(L2aArgs a)
{
    if (a.t.ctl[0] != 0) return;
    const uint64_t s = (uint64_t)blockIdx.x * kLT + threadIdx.x;
    const bool in = s < a.n_samples;
    uint64_t v[3] = {0, 0, 0};
    if (in) { v[0] = a.samp[2 * s]; v[1] = a.samp[2 * s + 1]; }
    uint64_t off[3], tot[3];
    block_scan<3, kLT>(v, off, tot);
    if (!in) return;
    const unsigned long long* p = a.part + (uint64_t)blockIdx.x * 8;
    uint64_t o = off[0] + p[0], r = off[1] + p[1];
    if (a.sample_off_out) a.sample_off_out[s] = o;
    const uint32_t sc = a.t.prefix;
    unsigned long long* const piece_out = a.t.piece_out;
    unsigned long long* const piece_delta = a.t.piece_delta;
    uint64_t recs, pay;
    (void)walk_sample(a, s, recs, pay, [&](uint64_t src, uint64_t len) {
        piece_out[r] = o;
        piece_delta[r] = src - (o + sc);
        o += sc + len; r += 1;
    });
}

} // namespace

hipError_t launch_annexb_to_lenpref(const A2lArgs& a, hipStream_t st)
{
    const uint64_t blocks = (a.n_nals + kLenprefNalsPerBlock - 1) / kLenprefNalsPerBlock;
    const hipError_t e = begin_launches(a.ev_begin, st);
    if (e != hipSuccess) return e;
    if (blocks) hipLaunchKernelGGL(k_a2l_count, dim3((unsigned)blocks), dim3(kLT), 0, st, a);
    hipLaunchKernelGGL(k_a2l_scan, dim3(1), dim3(kLT), 0, st, a, blocks);
    if (a.t.out && blocks) {
        hipLaunchKernelGGL(k_a2l_place, dim3((unsigned)blocks), dim3(kLT), 0, st, a);
        (void)copy_pieces(a.t, st);
    }
    return end_launches(a.ev_end, st);
}

hipError_t launch_lenpref_to_annexb(const L2aArgs& a, hipStream_t st)
{
    const uint64_t blocks = (a.n_samples + kLenprefSamplesPerBlock - 1) / kLenprefSamplesPerBlock;
    const hipError_t e = begin_launches(a.ev_begin, st);
    if (e != hipSuccess) return e;
    if (blocks) hipLaunchKernelGGL(k_l2a_count, dim3((unsigned)blocks), dim3(kLT), 0, st, a);
    hipLaunchKernelGGL(k_l2a_scan, dim3(1), dim3(kLT), 0, st, a, blocks);
    if (a.t.out && blocks) {
        hipLaunchKernelGGL(k_l2a_place, dim3((unsigned)blocks), dim3(kLT), 0, st, a);
        (void)copy_pieces(a.t, st);
    }
    return end_launches(a.ev_end, st);
}

} // namespace hbs
