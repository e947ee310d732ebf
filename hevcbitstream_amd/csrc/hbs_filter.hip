/*
 * hbs_filter.hip -- hbs_filter_annexb: cut an Annex-B stream down to some of its NAL units
 * (include/hevcbitstream_amd.h).  A plan of three launches and the copy's two, none of which waits for another workgroup:
 *
 *   k_filter_count   one lane per 8 consecutive NALs: check the entry, read its two header bytes, apply the
 *                    rule (or d_keep); per workgroup of 2048 NALs the sums of kept unit bytes, kept NALs, kept
 *                    rbsp_len, kept non-empty units, and whether an entry was inconsistent
 *   k_filter_scan    one workgroup: exclusive scan of those sums over the workgroups; totals, the error
 *                    (HBS_E_ARG, HBS_E_CAPACITY against out_cap) and the summary
 *   k_filter_place   the count again, now with the workgroup's offsets: the output index, and per kept non-empty
 *                    unit its output offset and its stream offset (minus the output offset), in kept order
 *   copy_pieces      (hbs_pieces.hip) a kept non-empty unit is a piece with a prefix of no bytes: a lane per 64 KiB output
 *                    tile finds the unit its first byte lies in, then a workgroup per tile copies.  A unit of any size spreads
 *                    over the tiles it covers.
 *
 * Traffic: the kept units read once and written once, the index read twice (32 B a NAL, count and place), 32 B a
 * kept NAL of output index, 16 B a kept unit of scratch written and read, 8 B a tile.
 */
#include <hip/hip_runtime.h>
#include "hbs_filter.h"
#include "hbs_plan.h"

namespace hbs {
namespace {

constexpr int kFT = kPlanLanes;                                       /* lanes of the plan workgroups */
constexpr int kFPer = kFilterNalsPerBlock / kFT;                      /* NALs a plan lane takes       */

struct Nal {
    uint64_t u, start, end;      /* unit [u, end); payload [start, end) */
    uint32_t rbsp_len;
    int32_t status;
    bool bad, kept;
};

/* entry k with the end of entry k-1 (0 for k = 0): checked before its header bytes are read */
__device__ __forceinline__ Nal eval_nal(const FilterArgs& a, uint64_t k, uint64_t prev_end)
{
    const hbs_nal_entry e = a.index[k];
    Nal r;
    r.u = prev_end; r.start = e.start; r.end = e.end; r.rbsp_len = e.rbsp_len; r.status = e.status;
    r.bad = e.start > e.end || e.end > a.n || e.start < prev_end;
    bool keep = false;
    if (!r.bad) {
        if (!a.use_rule) {
            keep = a.keep[k] != 0;
        } else if (e.end - e.start < 2) {
            keep = a.rule.keep_short != 0;
        } else {
            const uint32_t b0 = a.t.src[e.start], b1 = a.t.src[e.start + 1];
            const uint32_t type = (b0 >> 1) & 63u;
            const int32_t layer = (int32_t)(((b0 & 1u) << 5) | (b1 >> 3));
            const int32_t tid1 = (int32_t)(b1 & 7u);
            keep = ((a.rule.keep_types >> type) & 1ull) && tid1 <= a.rule.max_temporal_id_plus1 && layer <= a.rule.max_layer_id;
        }
    }
    r.kept = keep;
    return r;
}

__global__ __launch_bounds__(kFT) void k_filter_count(FilterArgs a)
{
    const uint64_t base = (uint64_t)blockIdx.x * kFilterNalsPerBlock + (uint64_t)threadIdx.x * kFPer;
    uint64_t v[4] = {0, 0, 0, 0};
    bool bad = false;
    if (base < a.n_nals) {
        uint64_t prev = base ? a.index[base - 1].end : 0;
        for (int i = 0; i < kFPer && base + i < a.n_nals; ++i) {
            const Nal x = eval_nal(a, base + i, prev);
            prev = x.end;
            bad |= x.bad;
            if (x.kept) {
                const uint64_t unit = x.end - x.u;
                v[0] += unit; v[1] += 1; v[2] += x.rbsp_len; v[3] += unit ? 1 : 0;
            }
        }
    }
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    uint64_t ex[4], tot[4];
    block_scan<4, kFT>(v, ex, tot);
    if (threadIdx.x == 0) {
        unsigned long long* p = a.part + (uint64_t)blockIdx.x * 8;
        p[0] = tot[0]; p[1] = tot[1]; p[2] = tot[2]; p[3] = tot[3]; p[4] = any_bad ? 1 : 0;
    }
}

__global__ __launch_bounds__(kFT) void k_filter_scan(FilterArgs a, uint64_t blocks)
{
    uint64_t carry[4];
    const uint64_t bad = scan_parts<4>(a.part, blocks, carry);
    if (threadIdx.x == 0) {
        const uint64_t total = carry[0], kept = carry[1], rbsp = carry[2], units = carry[3];
        const int32_t err = bad ? HBS_E_ARG : (a.t.out && total > a.out_cap) ? HBS_E_CAPACITY : 0;
        a.t.ctl[0] = (unsigned long long)(uint32_t)err;
        a.t.ctl[1] = total; a.t.ctl[2] = units; a.t.ctl[3] = kept;
        if (!err && a.t.out) a.t.piece_out[units] = total;
        hbs_summary s;
        s.nal_count = kept; s.nal_found = a.n_nals; s.rbsp_bytes = rbsp; s.stream_bytes = total;
        s.stop_reason = kept ? -1 : 0; s.error = err;
        s.reserved[0] = s.reserved[1] = s.reserved[2] = 0;
        *a.summary = s;
    }
}

__global__ __launch_bounds__(kFT) void k_filter_place(FilterArgs a)
{
    if (a.t.ctl[0] != 0) return;
    const uint64_t base = (uint64_t)blockIdx.x * kFilterNalsPerBlock + (uint64_t)threadIdx.x * kFPer;
    const uint64_t prev0 = (base && base < a.n_nals) ? a.index[base - 1].end : 0;
    uint64_t v[4] = {0, 0, 0, 0};
    if (base < a.n_nals) {
        uint64_t prev = prev0;
        for (int i = 0; i < kFPer && base + i < a.n_nals; ++i) {
            const Nal x = eval_nal(a, base + i, prev);
            prev = x.end;
            if (x.kept) {
                const uint64_t unit = x.end - x.u;
                v[0] += unit; v[1] += 1; v[2] += x.rbsp_len; v[3] += unit ? 1 : 0;
            }
        }
    }
    uint64_t off[4], tot[4];
    block_scan<4, kFT>(v, off, tot);
    if (base >= a.n_nals) return;
    const unsigned long long* p = a.part + (uint64_t)blockIdx.x * 8;
#pragma unroll
    for (int q = 0; q < 4; ++q) off[q] += p[q];
    const uint64_t last = a.t.ctl[3] - 1;          /* rank of the last kept NAL */
    uint64_t prev = prev0;
    for (int i = 0; i < kFPer && base + i < a.n_nals; ++i) {
        const Nal x = eval_nal(a, base + i, prev);
        prev = x.end;
        if (!x.kept) continue;
        const uint64_t unit = x.end - x.u;
        if (a.index_out) {
            hbs_nal_entry o;
            o.start = off[0] + (x.start - x.u);
            o.end = off[0] + unit;
            o.rbsp_off = off[2];
            o.rbsp_len = x.rbsp_len;
            o.status = (x.status & ~HBS_ST_UNTERMINATED) | (off[1] == last ? HBS_ST_UNTERMINATED : 0);
            a.index_out[off[1]] = o;
        }
        if (unit) {
            a.t.piece_out[off[3]] = off[0];
            a.t.piece_delta[off[3]] = x.u - off[0];
            off[3] += 1;
        }
        off[0] += unit; off[1] += 1; off[2] += x.rbsp_len;
    }
}

} // namespace

hipError_t launch_filter_annexb(const FilterArgs& a, hipStream_t st)
{
    const uint64_t blocks = (a.n_nals + kFilterNalsPerBlock - 1) / kFilterNalsPerBlock;
    const hipError_t e = begin_launches(a.ev_begin, st);
    if (e != hipSuccess) return e;
    if (blocks) hipLaunchKernelGGL(k_filter_count, dim3((unsigned)blocks), dim3(kFT), 0, st, a);
    hipLaunchKernelGGL(k_filter_scan, dim3(1), dim3(kFT), 0, st, a, blocks);
    if (a.t.out && blocks) {
        hipLaunchKernelGGL(k_filter_place, dim3((unsigned)blocks), dim3(kFT), 0, st, a);
        (void)copy_pieces(a.t, st);
    }
    return end_launches(a.ev_end, st);
}

} // namespace hbs
