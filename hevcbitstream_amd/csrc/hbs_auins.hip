/*
 * hbs_auins.hip -- hbs_au_insert: access-unit delimiters and copies of the parameter sets in force in front of the access
 * units of a range (include/hevcbitstream_amd.h is the specification, hbs_auins.h the AUD rule).  A plan of four launches, two
 * that place and the copy's two, none of which waits for another workgroup.  The NAL side takes 2048 consecutive NALs a
 * workgroup (8 a lane), the AU side 256 AUs a workgroup (one a lane); neither walks the other's records: an AU of any number
 * of NALs costs its lane the same.
 *
 *   k_auins_nals        NAL side, positions 0 .. n_nals: checks the index entry and d_nal_au[k]; "the last VPS / SPS / PPS in
 *                       front of position p" is an exclusive max-scan of `number + 1` (block_excl_max, hbs_plan.h), of which the workgroup
 *                       leaves its aggregate and, for every p that is an AU's picture NAL (or its end, without a picture), the
 *                       in-workgroup value with that AU; the sum of rbsp_len over the range's NALs
 *   k_auins_nal_scan    one workgroup: the aggregates become what lies in front of each NAL workgroup
 *   k_auins_aus         AU side, all AUs: checks the record against its neighbour and the index (before anything of it is
 *                       used as a number); for the AUs of the range decides, once, what is inserted (AuinsDec) and leaves
 *                       inserted bytes, AUDs, sets, AUs with insertions and inserted rbsp_len per workgroup
 *   k_auins_scan        one workgroup: scan_parts (hbs_plan.h) turns the sums into offsets; totals, the error, the summary
 *   k_auins_place_aus   AU side, the range: the piece table (the verbatim bytes between two AUs with insertions are ONE piece),
 *                       d_au_out, and where the NAL side finds the AU's offsets (AuinsPl)
 *   k_auins_place_nals  NAL side: d_index_out, d_nal_src, d_nal_au_out; the lane of an AU's first NAL also writes the entries
 *                       of what was inserted there
 *   copy_pieces         (hbs_pieces.hip) with a literal a piece: 7 bytes and no payload for an AUD, 4 and the payload for a
 *                       set, none for verbatim bytes
 *
 * Traffic: the range's bytes and the inserted sets read once and written once; per NAL 32 B of index twice, 32 B of d_parsed
 * and 4 B of d_nal_au (twice), 40 B of output tables; per AU 64 B twice, 80 B of scratch, 64 B of d_au_out; 24 B a piece.
 */
#include <hip/hip_runtime.h>
#include "hbs_auins.h"
#include "hbs_plan.h"

namespace hbs {
namespace {

constexpr int kT = kPlanLanes;
constexpr int kPer = kAuinsNalsPerBlock / kT;        /* NALs a lane of the NAL side takes */
static_assert(kAuinsAusPerBlock == kT, "one AU a lane");

/* the NALs of the range as the AU table names them: compared with, never used as an index before k_auins_aus has checked it */
__device__ __forceinline__ void range_nals(const AuinsArgs& a, uint64_t& k0, uint64_t& k1)
{
    k0 = k1 = 0;
    if (!a.cnt) return;
    k0 = a.au[a.a0].first_nal;
    k1 = a.au[a.a0 + a.cnt - 1].first_nal + a.au[a.a0 + a.cnt - 1].nal_count;
}

__device__ __forceinline__ int set_kind(const hbs_parsed_nal& p)
{
    return (p.rc >= 0 && p.nal_unit_type >= 32 && p.nal_unit_type <= 34) ? p.nal_unit_type - 31 : 0;      /* 1..3, 0: no set */
}

__global__ __launch_bounds__(kT) void k_auins_nals(AuinsArgs a)
{
    const uint64_t base = (uint64_t)blockIdx.x * kAuinsNalsPerBlock + (uint64_t)threadIdx.x * kPer;
    uint64_t k0, k1;
    range_nals(a, k0, k1);
    uint32_t m[3] = {0, 0, 0}, kinds = 0;
    uint64_t rb[1] = {0};
    bool bad = false;
    if (base < a.n_nals) {
        uint64_t prev = base ? a.index[base - 1].end : 0;
        for (int i = 0; i < kPer && base + i < a.n_nals; ++i) {
            const uint64_t k = base + i;
            const hbs_nal_entry e = a.index[k];
            bad |= e.start > e.end || e.end > a.n || e.start < prev;
            prev = e.end;
            if (k >= k0 && k < k1) rb[0] += e.rbsp_len;
            const uint32_t ai = a.nal_au[k];
            if (ai >= a.n_aus) bad = true;
            else {
                const uint64_t f = a.au[ai].first_nal;
                bad |= !(f <= k && k - f < (uint64_t)a.au[ai].nal_count);
            }
            const int kind = set_kind(a.parsed[k]);
            kinds |= (uint32_t)kind << (2 * i);
            if (kind) m[kind - 1] = (uint32_t)k + 1u;
        }
    }
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    uint32_t cur[3], tot[3];
    block_excl_max<uint32_t, 3, kT>(m, cur, tot);
    uint64_t rex[1], rtot[1];
    block_scan<1, kT>(rb, rex, rtot);
    if (threadIdx.x == 0) {
        a.part_n[(uint64_t)blockIdx.x * 8] = rtot[0];
        a.part_n[(uint64_t)blockIdx.x * 8 + 1] = any_bad ? 1 : 0;
        uint32_t* l = a.last_n + (uint64_t)blockIdx.x * 4;
        l[0] = tot[0]; l[1] = tot[1]; l[2] = tot[2]; l[3] = 0;
    }
    /* the positions an AU asks at: its picture NAL, or one past its last NAL when it has no picture */
    for (int i = 0; i < kPer && base + i <= a.n_nals; ++i) {
        const uint64_t k = base + i;
        if (k < a.n_nals) {
            const uint32_t ai = a.nal_au[k];
            if (ai < a.n_aus) {
                const uint64_t f = a.au[ai].first_nal;
                const uint32_t fv = a.au[ai].first_vcl;
                if (fv != ~0u && f + fv == k) { uint32_t* q = a.au_q + (uint64_t)ai * 4; q[0] = cur[0]; q[1] = cur[1]; q[2] = cur[2]; }
                if (f == k && ai > 0 && a.au[ai - 1].first_vcl == ~0u) { uint32_t* q = a.au_q + (uint64_t)(ai - 1) * 4; q[0] = cur[0]; q[1] = cur[1]; q[2] = cur[2]; }
            }
            const uint32_t kind = (kinds >> (2 * i)) & 3u;
            if (kind) cur[kind - 1] = (uint32_t)k + 1u;
        } else if (a.au[a.n_aus - 1].first_vcl == ~0u) {
            uint32_t* q = a.au_q + (a.n_aus - 1) * 4; q[0] = cur[0]; q[1] = cur[1]; q[2] = cur[2];
        }
    }
}

/* ctl2: 0 first NAL of the range, 1 one past its last, 2 unit_begin of its first AU, 3 M, 4 rbsp_len of the range's NALs,
 * 5 the NAL side found something inconsistent */
__global__ __launch_bounds__(kT) void k_auins_nal_scan(AuinsArgs a, uint64_t blocks)
{
    uint64_t carry[1];
    const uint64_t bad = scan_parts<1>(a.part_n, blocks, carry);
    uint32_t run[3] = {0, 0, 0};
    for (uint64_t seg = 0; seg < blocks; seg += (uint64_t)kT * kPlanPer) {
        const uint64_t i0 = seg + (uint64_t)threadIdx.x * kPlanPer;
        uint32_t acc[3] = {0, 0, 0};
        for (int i = 0; i < kPlanPer && i0 + i < blocks; ++i)
#pragma unroll
            for (int q = 0; q < 3; ++q) acc[q] = max(acc[q], a.last_n[(i0 + i) * 4 + q]);
        uint32_t cur[3], tot[3];
        block_excl_max<uint32_t, 3, kT>(acc, cur, tot);
#pragma unroll
        for (int q = 0; q < 3; ++q) cur[q] = max(cur[q], run[q]);
        for (int i = 0; i < kPlanPer && i0 + i < blocks; ++i)
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const uint32_t x = a.last_n[(i0 + i) * 4 + q];
                a.last_n[(i0 + i) * 4 + q] = cur[q];
                cur[q] = max(cur[q], x);
            }
#pragma unroll
        for (int q = 0; q < 3; ++q) run[q] = max(run[q], tot[q]);
    }
    if (threadIdx.x == 0) { a.ctl2[4] = carry[0]; a.ctl2[5] = bad; }
}

__device__ __forceinline__ uint32_t dec_sets(const AuinsDec& d) { return (d.q[0] ? 1u : 0u) + (d.q[1] ? 1u : 0u) + (d.q[2] ? 1u : 0u); }

__global__ __launch_bounds__(kT) void k_auins_aus(AuinsArgs a)
{
    const uint64_t i = (uint64_t)blockIdx.x * kAuinsAusPerBlock + threadIdx.x;
    uint64_t v[5] = {0, 0, 0, 0, 0};
    bool bad = false;
    if (i < a.n_aus) {
        const hbs_access_unit r = a.au[i];
        const uint64_t f = r.first_nal, c = r.nal_count;
        bool ok = c >= 1 && f < a.n_nals && c <= a.n_nals - f && (i != 0 || f == 0) && (r.first_vcl == ~0u || r.first_vcl < c);
        if (ok) {
            const uint64_t next = i + 1 < a.n_aus ? a.au[i + 1].first_nal : a.n_nals;
            ok = next == f + c && r.unit_begin == (f ? a.index[f - 1].end : 0) && r.unit_end == a.index[f + c - 1].end;
        }
        bad = !ok;
        if (ok && i >= a.a0 && i - a.a0 < a.cnt) {
            const bool own_aud = a.parsed[f].nal_unit_type == 35;
            const bool aud = (a.flags & HBS_AUINS_AUD) && !(r.flags & HBS_AU_NO_PICTURE) && !own_aud;
            const bool sets = ((a.flags & HBS_AUINS_PARAM_SETS) && (r.flags & HBS_AU_IRAP)) || ((a.flags & HBS_AUINS_PARAM_SETS_FIRST) && i == a.a0);
            AuinsDec d;
            d.q[0] = d.q[1] = d.q[2] = 0;
            d.bits = (aud ? 1u : 0u) | (own_aud ? 2u : 0u);
            d.ins_bytes = aud ? kAuinsAudBytes : 0; d.ins_rbsp = aud ? 3 : 0;
            if (sets) {
                const uint64_t p = f + (r.first_vcl == ~0u ? c : (uint64_t)r.first_vcl);
                const uint32_t* before = a.last_n + p / kAuinsNalsPerBlock * 4;
#pragma unroll
                for (int t = 0; t < 3; ++t) {
                    const uint32_t qv = max(before[t], a.au_q[i * 4 + t]);
                    if ((uint64_t)qv > p) { bad = true; continue; }          /* (never with tables that tile: nobody wrote au_q) */
                    if (qv == 0 || (uint64_t)qv - 1 >= f) continue;             /* none, or the AU brings its own */
                    const hbs_nal_entry e = a.index[qv - 1];
                    d.q[t] = qv; d.ins_bytes += 4 + (e.end - e.start); d.ins_rbsp += e.rbsp_len;
                }
            }
            a.dec[i] = d;
            const uint32_t ns = dec_sets(d);
            v[0] = d.ins_bytes; v[1] = aud ? 1 : 0; v[2] = ns; v[3] = (aud || ns) ? 1 : 0; v[4] = d.ins_rbsp;
        }
    }
    const int any_bad = __syncthreads_or(bad ? 1 : 0);
    uint64_t ex[5], tot[5];
    block_scan<5, kT>(v, ex, tot);
    if (threadIdx.x == 0) {
        unsigned long long* p = a.part_a + (uint64_t)blockIdx.x * 8;
        p[0] = tot[0]; p[1] = tot[1]; p[2] = tot[2]; p[3] = tot[3]; p[4] = tot[4]; p[5] = any_bad ? 1 : 0;
    }
}

/* blocks 0: n_nals or n_aus is 0, nothing was looked at */
__global__ __launch_bounds__(kT) void k_auins_scan(AuinsArgs a, uint64_t blocks)
{
    uint64_t carry[5];
    const uint64_t bad_a = scan_parts<5>(a.part_a, blocks, carry);
    if (threadIdx.x != 0) return;
    const bool bad = blocks && (bad_a || a.ctl2[5]);
    uint64_t bytes = 0, M = 0, rbsp = 0, pieces = 0, k0 = 0, k1 = 0, ub0 = 0;
    if (blocks && a.cnt && !bad) {
        const hbs_access_unit* first = a.au + a.a0;
        const hbs_access_unit* last = a.au + a.a0 + a.cnt - 1;
        k0 = first->first_nal; k1 = last->first_nal + last->nal_count; ub0 = first->unit_begin;
        bytes = last->unit_end - ub0 + carry[0];
        M = k1 - k0 + carry[1] + carry[2];
        rbsp = a.ctl2[4] + carry[4];
        pieces = 1 + carry[1] + carry[2] + carry[3];
    }
    const bool tables = a.index_out || a.nal_src || a.nal_au_out;
    const int32_t err = bad ? HBS_E_ARG : ((a.t.out && bytes > a.out_cap) || (tables && M > a.index_cap)) ? HBS_E_CAPACITY : 0;
    a.t.ctl[0] = (unsigned long long)(uint32_t)err;
    a.t.ctl[1] = bytes; a.t.ctl[2] = pieces;
    if (!err && a.t.out && pieces) a.t.piece_out[pieces] = bytes;
    a.ctl2[0] = k0; a.ctl2[1] = k1; a.ctl2[2] = ub0; a.ctl2[3] = M;
    hbs_summary s;
    s.nal_count = M; s.nal_found = a.n_nals; s.rbsp_bytes = rbsp; s.stream_bytes = bytes;
    s.stop_reason = M ? -1 : 0; s.error = err;
    s.reserved[0] = bad ? 0 : carry[1]; s.reserved[1] = bad ? 0 : carry[2]; s.reserved[2] = (bad || !blocks) ? 0 : a.cnt;
    *a.summary = s;
}

__global__ __launch_bounds__(kT) void k_auins_place_aus(AuinsArgs a, uint64_t block0)
{
    if (a.t.ctl[0] != 0) return;
    const uint64_t blk = block0 + blockIdx.x;
    const uint64_t i = blk * kAuinsAusPerBlock + threadIdx.x;
    const bool in = i >= a.a0 && i - a.a0 < a.cnt;
    AuinsDec d;
    d.q[0] = d.q[1] = d.q[2] = 0; d.bits = 0; d.ins_bytes = 0; d.ins_rbsp = 0;
    if (in) d = a.dec[i];
    const uint32_t ns = dec_sets(d), ins_n = (d.bits & 1u) + ns;
    const uint64_t v[5] = {d.ins_bytes, d.bits & 1u, ns, ins_n ? 1u : 0u, d.ins_rbsp};
    uint64_t ex[5], tot[5];
    block_scan<5, kT>(v, ex, tot);
    if (!in) return;
    const unsigned long long* part = a.part_a + blk * 8;
#pragma unroll
    for (int q = 0; q < 5; ++q) ex[q] += part[q];
    const hbs_access_unit r = a.au[i];
    const uint64_t k0 = a.ctl2[0], ub0 = a.ctl2[2], f = r.first_nal;
    const uint64_t base_out = r.unit_begin - ub0 + ex[0];
    const uint64_t I = (d.bits & 2u) ? a.index[f].end : r.unit_begin;           /* the insertion point */
    AuinsPl pl;
    pl.ex_bytes = ex[0]; pl.ex_rbsp = ex[4]; pl.ex_nals = (uint32_t)(ex[1] + ex[2]); pl.first_nal = (uint32_t)f; pl.pad[0] = pl.pad[1] = 0;
    a.pl[i] = pl;
    if (i == a.a0) { a.t.piece_out[0] = 0; a.t.piece_delta[0] = ub0; a.t.piece_lit[0] = 0; }
    if (ins_n) {
        uint64_t pj = 1 + ex[1] + ex[2] + ex[3], o = base_out + (I - r.unit_begin);
        if (d.bits & 1u) {
            a.t.piece_out[pj] = o; a.t.piece_delta[pj] = 0;
            a.t.piece_lit[pj] = ((unsigned long long)kAuinsAudBytes << 56) | auins_aud_word(r.temporal_id_plus1, r.slice_types);
            pj += 1; o += kAuinsAudBytes;
        }
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            if (!d.q[t]) continue;
            const hbs_nal_entry e = a.index[d.q[t] - 1];
            a.t.piece_out[pj] = o; a.t.piece_delta[pj] = e.start - (o + 4);
            a.t.piece_lit[pj] = (4ull << 56) | 0x01000000ull;                  /* 00 00 00 01 */
            pj += 1; o += 4 + (e.end - e.start);
        }
        a.t.piece_out[pj] = o; a.t.piece_delta[pj] = I - o; a.t.piece_lit[pj] = 0;      /* the bytes up to the next insertion */
    }
    if (a.au_out) {
        hbs_access_unit w = r;
        w.first_nal = f - k0 + pl.ex_nals;
        w.unit_begin = base_out;
        w.unit_end = base_out + (r.unit_end - r.unit_begin) + d.ins_bytes;
        w.nal_count = r.nal_count + ins_n;
        if (r.first_vcl != ~0u) w.first_vcl = r.first_vcl + ins_n;
        if (ns) w.flags |= HBS_AU_PARAM_SETS;
        a.au_out[i - a.a0] = w;
    }
}

__device__ __forceinline__ void put_nal(const AuinsArgs& a, uint64_t j, const hbs_nal_entry& o, uint32_t src, uint32_t au)
{
    if (a.index_out) a.index_out[j] = o;
    if (a.nal_src) a.nal_src[j] = src;
    if (a.nal_au_out) a.nal_au_out[j] = au;
}

__global__ __launch_bounds__(kT) void k_auins_place_nals(AuinsArgs a)
{
    if (a.t.ctl[0] != 0) return;
    const uint64_t k0 = a.ctl2[0], k1 = a.ctl2[1], ub0 = a.ctl2[2], last = a.ctl2[3] - 1;
    const uint64_t blk_lo = (uint64_t)blockIdx.x * kAuinsNalsPerBlock;
    if (blk_lo >= k1 || blk_lo + kAuinsNalsPerBlock <= k0) return;
    const uint64_t base = blk_lo + (uint64_t)threadIdx.x * kPer;
    uint64_t v[1] = {0};
    for (int i = 0; i < kPer; ++i) {
        const uint64_t k = base + i;
        if (k >= k0 && k < k1) v[0] += a.index[k].rbsp_len;
    }
    uint64_t ex[1], tot[1];
    block_scan<1, kT>(v, ex, tot);
    uint64_t rb = ex[0] + a.part_n[(uint64_t)blockIdx.x * 8];
    for (int i = 0; i < kPer; ++i) {
        const uint64_t k = base + i;
        if (k < k0 || k >= k1) continue;
        const hbs_nal_entry e = a.index[k];
        const uint32_t ai = a.nal_au[k], au_no = (uint32_t)(ai - a.a0);
        const AuinsDec d = a.dec[ai];
        const AuinsPl pl = a.pl[ai];
        const uint32_t ns = dec_sets(d), ins_n = (d.bits & 1u) + ns;
        const bool own_aud = (d.bits & 2u) != 0, head = k == pl.first_nal;
        const bool shifted = !(head && own_aud);                    /* an AUD of the AU's own stays in front of the insertions */
        const uint64_t at = k - k0 + pl.ex_nals;
        if (head && ins_n) {
            uint64_t j = at + (own_aud ? 1 : 0), rbi = rb + pl.ex_rbsp + (own_aud ? e.rbsp_len : 0);
            uint64_t o = (own_aud ? e.end : (k ? a.index[k - 1].end : 0)) - ub0 + pl.ex_bytes;
            if (d.bits & 1u) {
                hbs_nal_entry x;
                x.start = o + 4; x.end = o + kAuinsAudBytes; x.rbsp_off = rbi; x.rbsp_len = 3; x.status = 0;
                put_nal(a, j, x, 0xFFFFFFFFu, au_no);
                j += 1; o += kAuinsAudBytes; rbi += 3;
            }
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                if (!d.q[t]) continue;
                const hbs_nal_entry s = a.index[d.q[t] - 1];
                hbs_nal_entry x;
                x.start = o + 4; x.end = x.start + (s.end - s.start); x.rbsp_off = rbi; x.rbsp_len = s.rbsp_len;
                x.status = (s.status & ~HBS_ST_UNTERMINATED) | (j == last ? HBS_ST_UNTERMINATED : 0);
                put_nal(a, j, x, d.q[t] - 1u, au_no);
                j += 1; o = x.end; rbi += s.rbsp_len;
            }
        }
        const uint64_t j = at + (shifted ? ins_n : 0), shift = pl.ex_bytes + (shifted ? d.ins_bytes : 0) - ub0;
        hbs_nal_entry x;
        x.start = e.start + shift; x.end = e.end + shift;
        x.rbsp_off = rb + pl.ex_rbsp + (shifted ? d.ins_rbsp : 0); x.rbsp_len = e.rbsp_len;
        x.status = (e.status & ~HBS_ST_UNTERMINATED) | (j == last ? HBS_ST_UNTERMINATED : 0);
        put_nal(a, j, x, (uint32_t)k, au_no);
        rb += e.rbsp_len;
    }
}

} // namespace

hipError_t launch_au_insert(const AuinsArgs& a, hipStream_t st)
{
    const bool any = a.n_nals && a.n_aus;
    const uint64_t blocks_n = auins_nal_blocks(a.n_nals), blocks_a = auins_au_blocks(a.n_aus);
    const hipError_t e = begin_launches(a.ev_begin, st);
    if (e != hipSuccess) return e;
    if (any) {
        hipLaunchKernelGGL(k_auins_nals, dim3((unsigned)blocks_n), dim3(kT), 0, st, a);
        hipLaunchKernelGGL(k_auins_nal_scan, dim3(1), dim3(kT), 0, st, a, blocks_n);
        hipLaunchKernelGGL(k_auins_aus, dim3((unsigned)blocks_a), dim3(kT), 0, st, a);
    }
    hipLaunchKernelGGL(k_auins_scan, dim3(1), dim3(kT), 0, st, a, any ? blocks_a : 0);
    if (any && a.cnt && a.t.out) {
        const uint64_t b0 = a.a0 / kAuinsAusPerBlock, b1 = (a.a0 + a.cnt - 1) / kAuinsAusPerBlock;
        hipLaunchKernelGGL(k_auins_place_aus, dim3((unsigned)(b1 - b0 + 1)), dim3(kT), 0, st, a, b0);
        if (a.index_out || a.nal_src || a.nal_au_out) hipLaunchKernelGGL(k_auins_place_nals, dim3((unsigned)blocks_n), dim3(kT), 0, st, a);
        (void)copy_pieces(a.t, st);
    }
    return end_launches(a.ev_end, st);
}

} // namespace hbs
