/*
 * hbs_au.hip -- hbs_access_units: group the NALs of an indexed, parsed stream into access units and give every picture
 * its PicOrderCntVal; hbs_au_keep: from a range of access units to the keep mask of hbs_filter_annexb
 * (include/hevcbitstream_amd.h is the specification, hbs_au.h the rules).  Eight launches, none of which waits for
 * another workgroup; a workgroup takes 2048 consecutive NALs, one NAL per lane in eight steps:
 *
 *   k_au_digest   reads the three records of a NAL (96 B, whole 16-byte loads) and the SPS word of an SPS NAL, leaves a
 *                 16-byte digest (class bits, poc lsb, end) and per workgroup the last VCL / CAND / EOS / SPS NAL
 *   k_au_scan1    one workgroup: exclusive max-scan of those over the workgroups
 *   k_au_group    digest + prefixes: AU starts and picture NALs; per workgroup their counts, the last start, picture, anchor
 *   k_au_scan2    scan of those; the AU count against au_cap
 *   k_au_poc      per picture: CVS start (the EOS rule), Max from its SPS, the anchor in front, d(p); the verdicts go into
 *                 the digest's spare bits; per workgroup the segmented sum of d over its anchors
 *   k_au_scan3    scan of those; summary and carry
 *   k_au_write    d_nal_au, and the AU records: a forward segmented scan (segments begin at AU starts) brings count, VCL
 *                 count, flags, slice types, picture NAL and POC to the last NAL the AU has in the workgroup, which stores
 *                 the record -- or, when the AU began in an earlier workgroup, the workgroup's share of it
 *   k_au_fix      one lane per workgroup: adds that share to the record (an AU may span any number of workgroups)
 *
 * Traffic: 96 B a NAL read once, the digest written once (16 B) and read three times, 4 B of it rewritten, 4 B a NAL of
 * d_nal_au, 64 B an AU.
 */
#include <hip/hip_runtime.h>
#include "hbs_au.h"
#include "hbs_wave.h"

namespace hbs {
namespace {

constexpr int kT = 256;
constexpr int kSteps = kAuNalsPerBlock / kT;

/* verdicts k_au_poc leaves in the digest's class word */
constexpr uint32_t AU_C_START = 1u << 21, AU_C_PIC = 1u << 22, AU_C_CVS = 1u << 23;
constexpr int AU_C_DSIGN_SHIFT = 24;                 /* 2 bits: d(p) is 0 / +Max / -Max */
constexpr int AU_C_DLOG_SHIFT = 26;                  /* 4 bits: log2(Max) - 4           */

/* A scan of N 32-bit fields over the lanes of a workgroup.  Field q is a maximum (bit q of kMax), a bitwise or (kOr) or
 * a sum; 0 is the identity of all three.  Fields in kSeg restart at an element with a head (au_seg_combine). */
template <int N, uint32_t kMax, uint32_t kOr, uint32_t kSeg>
struct Scan {
    static __device__ __forceinline__ uint32_t op(int q, uint32_t a, uint32_t b)
    {
        return ((kMax >> q) & 1u) ? (a > b ? a : b) : ((kOr >> q) & 1u) ? (a | b) : a + b;
    }
    /* b = a o b (a in front) */
    static __device__ __forceinline__ void comb(const uint32_t a[N], uint32_t ha, uint32_t b[N], uint32_t& hb)
    {
#pragma unroll
        for (int q = 0; q < N; ++q)
            if (!(((kSeg >> q) & 1u) && hb)) b[q] = op(q, a[q], b[q]);
        hb |= ha;
    }
    template <int kCtrl, int kRowMask>
    static __device__ __forceinline__ void dpp_step(uint32_t x[N], uint32_t& hx)
    {
        uint32_t y[N];
#pragma unroll
        for (int q = 0; q < N; ++q) y[q] = dpp_or_zero<kCtrl, kRowMask>(x[q]);
        const uint32_t hy = dpp_or_zero<kCtrl, kRowMask>(hx);
        comb(y, hy, x, hx);
    }
    /* v, h: the lane's element.  inc / ex: everything in front of the workgroup (run) and the lanes up to and including /
     * in front of this one.  run becomes run o (all lanes). */
    static __device__ __forceinline__ void block(const uint32_t v[N], uint32_t h, uint32_t inc[N], uint32_t ex[N], uint32_t run[N], uint32_t& hrun)
    {
        __shared__ uint32_t s_w[kT / 64][N + 1];
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        uint32_t x[N], hx = h ? 1u : 0u;
#pragma unroll
        for (int q = 0; q < N; ++q) x[q] = v[q];
        /* the wave's inclusive scan with DPP moves as hbs_wave.h's wave_incl_scan32: a lane without a source reads 0, the
         * identity of every field and "no head" */
        dpp_step<kDppRowShr1, 0xF>(x, hx);
        dpp_step<kDppRowShr2, 0xF>(x, hx);
        dpp_step<kDppRowShr4, 0xF>(x, hx);
        dpp_step<kDppRowShr8, 0xF>(x, hx);
        dpp_step<kDppBcast15, 0xA>(x, hx);          /* rows 1 and 3 <- the total of the row in front */
        dpp_step<kDppBcast31, 0xC>(x, hx);          /* rows 2 and 3 <- the total of the first half   */
        uint32_t e[N], he = from_prev_lane(hx, 0u);
#pragma unroll
        for (int q = 0; q < N; ++q) e[q] = from_prev_lane(x[q], 0u);
        if (lane == 63) {
#pragma unroll
            for (int q = 0; q < N; ++q) s_w[wave][q] = x[q];
            s_w[wave][N] = hx;
        }
        __syncthreads();
        uint32_t p[N], hp = hrun, t[N], ht = hrun;
#pragma unroll
        for (int q = 0; q < N; ++q) { p[q] = run[q]; t[q] = run[q]; }
#pragma unroll
        for (int w = 0; w < kT / 64; ++w) {
            uint32_t wv[N], hw = s_w[w][N];
#pragma unroll
            for (int q = 0; q < N; ++q) wv[q] = s_w[w][q];
            if (w < wave) {
                uint32_t c[N], hc = hw;
#pragma unroll
                for (int q = 0; q < N; ++q) c[q] = wv[q];
                comb(p, hp, c, hc);
#pragma unroll
                for (int q = 0; q < N; ++q) p[q] = c[q];
                hp = hc;
            }
            comb(t, ht, wv, hw);
#pragma unroll
            for (int q = 0; q < N; ++q) t[q] = wv[q];
            ht = hw;
        }
        comb(p, hp, x, hx);
        comb(p, hp, e, he);
#pragma unroll
        for (int q = 0; q < N; ++q) { inc[q] = x[q]; ex[q] = e[q]; run[q] = t[q]; }
        hrun = ht;
        __syncthreads();
    }

    /* one workgroup: part[b * 8 + q] (head: part[b * 8 + 7]) of every block b becomes what lies in front of block b,
     * beginning with run; run becomes the total */
    static __device__ __forceinline__ void parts(uint32_t* part, uint64_t blocks, uint32_t run[N], uint32_t& hrun)
    {
        for (uint64_t seg = 0; seg < blocks; seg += (uint64_t)kT * kSteps) {
            const uint64_t i0 = seg + (uint64_t)threadIdx.x * kSteps;
            uint32_t acc[N], hacc = 0;
#pragma unroll
            for (int q = 0; q < N; ++q) acc[q] = 0;
            for (int i = 0; i < kSteps && i0 + i < blocks; ++i) {
                uint32_t el[N], hel = kSeg ? part[(i0 + i) * 8 + 7] : 0u;
#pragma unroll
                for (int q = 0; q < N; ++q) el[q] = part[(i0 + i) * 8 + q];
                comb(acc, hacc, el, hel);
#pragma unroll
                for (int q = 0; q < N; ++q) acc[q] = el[q];
                hacc = hel;
            }
            uint32_t inc[N], cur[N];
            uint32_t hcur = 0;
            block(acc, hacc, inc, cur, run, hrun);
            for (int i = 0; i < kSteps && i0 + i < blocks; ++i) {
                uint32_t el[N], hel = kSeg ? part[(i0 + i) * 8 + 7] : 0u;
#pragma unroll
                for (int q = 0; q < N; ++q) el[q] = part[(i0 + i) * 8 + q];
#pragma unroll
                for (int q = 0; q < N; ++q) part[(i0 + i) * 8 + q] = cur[q];
                comb(cur, hcur, el, hel);
#pragma unroll
                for (int q = 0; q < N; ++q) cur[q] = el[q];
                hcur = 0;       /* cur already carries what a head in front decided */
            }
        }
    }
};

typedef Scan<4, 0xFu, 0u, 0u> ScanLast4;             /* last VCL, CAND, EOS, SPS-with-slot NAL (number + 1) */
typedef Scan<2, 0x3u, 0u, 0u> ScanLast2;
typedef Scan<5, 0x0Fu, 0u, 0u> ScanPart1;            /* ... and the VCL count */
typedef Scan<5, 0x1Cu, 0u, 0u> ScanPart2;            /* AU starts, pictures | last start, picture, anchor */
typedef Scan<2, 0x2u, 0u, 0u> ScanStart;             /* AU starts | last start */
typedef Scan<2, 0u, 0u, 0x2u> ScanPart3;             /* CVS starts | segmented: the anchors' msb */
typedef Scan<1, 0u, 0u, 0x1u> ScanMsb;
typedef Scan<5, 0x8u, 0x4u, 0x1Fu> ScanAu;           /* per AU: NALs, VCL NALs, flags and slice types (or), picture NAL (max), POC */

__device__ __forceinline__ AuDigest load_digest(const AuDigest* d, uint64_t k)
{
    const u32x4 x = *reinterpret_cast<const u32x4*>(d + k);
    AuDigest r;
    r.cls = x.x; r.lsb = (int32_t)x.y; r.end = (uint64_t)x.z | ((uint64_t)x.w << 32);
    return r;
}

__global__ __launch_bounds__(kT) void k_au_digest(AuArgs a)
{
    const uint64_t base = (uint64_t)blockIdx.x * kAuNalsPerBlock;
    uint32_t agg[5] = {0, 0, 0, 0, 0};
    for (int s = 0; s < kSteps; ++s) {
        const uint64_t k = base + (uint64_t)s * kT + threadIdx.x;
        if (k >= a.n_nals) break;
        const u32x4* pp = reinterpret_cast<const u32x4*>(a.parsed + k);
        const u32x4* cp = reinterpret_cast<const u32x4*>(a.compact + k);
        const u32x4 p0 = pp[0], p1 = pp[1], c0 = cp[0], c1 = cp[1];
        const u32x4 i0 = *reinterpret_cast<const u32x4*>(a.index + k);
        const int32_t type = (int32_t)p0.y;
        const uint64_t struct_off = (uint64_t)p1.x | ((uint64_t)p1.y << 32);
        const bool slot = type == 33 && struct_off != ~0ull && a.structs != nullptr;
        const int32_t log2m4 = slot ? *reinterpret_cast<const int32_t*>(a.structs + struct_off + a.sps_off) : 0;
        const uint32_t cls = au_classify((int32_t)p0.x, type, (int32_t)p0.z, (int32_t)p0.w, slot ? 1 : 0, log2m4,
                                         (int32_t)c0.x, (int32_t)c0.w, (int32_t)c1.y);
        u32x4 d;
        d.x = cls; d.y = c1.w; d.z = i0.z; d.w = i0.w;
        *reinterpret_cast<u32x4*>(a.digest + k) = d;
        const uint32_t k1 = (uint32_t)k + 1u;
        if (au_is_vcl(cls)) { agg[0] = k1; agg[4] += 1; }
        if (au_is_cand(cls)) agg[1] = k1;
        if (au_is_eos(cls)) agg[2] = k1;
        if (cls & AU_C_SPS_SLOT) agg[3] = k1;
    }
    uint32_t inc[5], ex[5], run[5] = {0, 0, 0, 0, 0}, hrun = 0;
    ScanPart1::block(agg, 0, inc, ex, run, hrun);
    if (threadIdx.x == 0) {
        uint32_t* p = a.part1 + (uint64_t)blockIdx.x * 8;
        p[0] = run[0]; p[1] = run[1]; p[2] = run[2]; p[3] = run[3]; p[4] = run[4]; p[5] = 0; p[6] = 0; p[7] = 0;
    }
}

/* ctl: 0 error, 1 AUs, 2 pictures, 3 last picture, 4 last anchor, 5 last EOS (numbers + 1) */
__global__ __launch_bounds__(kT) void k_au_scan1(AuArgs a, uint64_t blocks)
{
    uint32_t run[5] = {0, 0, 0, 0, 0}, hrun = 0;
    ScanPart1::parts(a.part1, blocks, run, hrun);
    if (threadIdx.x == 0) a.ctl[5] = run[2];
}

__global__ __launch_bounds__(kT) void k_au_group(AuArgs a)
{
    const uint64_t base = (uint64_t)blockIdx.x * kAuNalsPerBlock;
    const uint32_t* p1 = a.part1 + (uint64_t)blockIdx.x * 8;
    uint32_t run[2] = {p1[0], p1[1]}, hrun = 0;
    uint32_t agg[5] = {0, 0, 0, 0, 0};
    for (int s = 0; s < kSteps; ++s) {
        const uint64_t k = base + (uint64_t)s * kT + threadIdx.x;
        const bool valid = k < a.n_nals;
        const uint32_t cls = valid ? a.digest[k].cls : 0u;
        const uint32_t k1 = (uint32_t)k + 1u;
        const uint32_t v[2] = {valid && au_is_vcl(cls) ? k1 : 0u, valid && au_is_cand(cls) ? k1 : 0u};
        uint32_t inc[2], ex[2];
        ScanLast2::block(v, 0, inc, ex, run, hrun);
        if (valid) {
            if (au_starts(cls, k, ex[0], ex[1])) { agg[0] += 1; agg[2] = k1; }
            if (au_is_picture(cls, ex[0], ex[1])) {
                agg[1] += 1; agg[3] = k1;
                if (au_picture_flags(cls) & HBS_AU_ANCHOR) agg[4] = k1;
            }
        }
    }
    uint32_t inc[5], ex[5], tot[5] = {0, 0, 0, 0, 0}, htot = 0;
    ScanPart2::block(agg, 0, inc, ex, tot, htot);
    if (threadIdx.x == 0) {
        uint32_t* p = a.part2 + (uint64_t)blockIdx.x * 8;
        p[0] = tot[0]; p[1] = tot[1]; p[2] = tot[2]; p[3] = tot[3]; p[4] = tot[4]; p[5] = 0; p[6] = 0; p[7] = 0;
    }
}

__global__ __launch_bounds__(kT) void k_au_scan2(AuArgs a, uint64_t blocks)
{
    uint32_t run[5] = {0, 0, 0, 0, 0}, hrun = 0;
    ScanPart2::parts(a.part2, blocks, run, hrun);
    if (threadIdx.x == 0) {
        a.ctl[0] = (a.au && (uint64_t)run[0] > a.au_cap) ? (uint32_t)HBS_E_CAPACITY : 0u;
        a.ctl[1] = run[0]; a.ctl[2] = run[1]; a.ctl[3] = run[3]; a.ctl[4] = run[4];
    }
}

__global__ __launch_bounds__(kT) void k_au_poc(AuArgs a)
{
    const uint64_t base = (uint64_t)blockIdx.x * kAuNalsPerBlock;
    const uint32_t* p1 = a.part1 + (uint64_t)blockIdx.x * 8;
    const uint32_t* p2 = a.part2 + (uint64_t)blockIdx.x * 8;
    uint32_t runA[4] = {p1[0], p1[1], p1[2], p1[3]}, hA = 0;
    uint32_t runB[2] = {p2[3], p2[4]}, hB = 0;
    uint32_t seg[1] = {0}, hseg = 0;                 /* the block's anchors: (reset, sum) */
    uint32_t cvs_count = 0;
    for (int s = 0; s < kSteps; ++s) {
        const uint64_t k = base + (uint64_t)s * kT + threadIdx.x;
        const bool valid = k < a.n_nals;
        AuDigest g;
        g.cls = 0; g.lsb = 0; g.end = 0;
        if (valid) g = load_digest(a.digest, k);
        const uint32_t cls = g.cls, k1 = (uint32_t)k + 1u;
        const uint32_t va[4] = {valid && au_is_vcl(cls) ? k1 : 0u, valid && au_is_cand(cls) ? k1 : 0u,
                                valid && au_is_eos(cls) ? k1 : 0u, (valid && (cls & AU_C_SPS_SLOT)) ? k1 : 0u};
        uint32_t incA[4], exA[4];
        ScanLast4::block(va, 0, incA, exA, runA, hA);
        const bool start = valid && au_starts(cls, k, exA[0], exA[1]);
        const bool pic = valid && au_is_picture(cls, exA[0], exA[1]);
        const bool anchor = pic && (au_picture_flags(cls) & HBS_AU_ANCHOR);
        const uint32_t vb[2] = {pic ? k1 : 0u, anchor ? k1 : 0u};
        uint32_t incB[2], exB[2];
        ScanLast2::block(vb, 0, incB, exB, runB, hB);
        bool cvs = false;
        int32_t d = 0;
        uint32_t log2m4 = 0;
        if (pic) {
            const bool pic_seen = exB[0] != 0 || (a.initial.flags & 1u);
            const bool eos_pending = exB[0] != 0 ? exA[2] > exB[0] : (exA[2] != 0 || (a.initial.flags & 4u));
            cvs = au_cvs_start(cls, pic_seen, eos_pending);
            if (exA[3]) log2m4 = (a.digest[exA[3] - 1].cls >> AU_C_LOG2_SHIFT) & 15u;
            const int32_t prev = exB[1] ? a.digest[exB[1] - 1].lsb : ((a.initial.flags & 2u) ? a.initial.anchor_poc_lsb : 0);
            d = au_poc_delta(prev, g.lsb, log2m4);
        }
        if (valid) {
            const uint32_t verdict = (start ? AU_C_START : 0u) | (pic ? AU_C_PIC : 0u) | (cvs ? AU_C_CVS : 0u) |
                                     ((d > 0 ? 1u : d < 0 ? 2u : 0u) << AU_C_DSIGN_SHIFT) | (log2m4 << AU_C_DLOG_SHIFT);
            /* Other workgroups read bits 17..20 of SPS NALs' class words (and the lsb words next to them) in this launch with
             * plain loads while this plain store rewrites the word: formally a race.  It is harmless because the store is one
             * aligned dword, which the hardware does not tear, and every bit below 21 keeps its value -- a reader gets the same
             * low bits from the old word and from the new one.  Nobody reads bits 21.. before the next launch. */
            a.digest[k].cls = cls | verdict;
        }
        cvs_count += cvs ? 1u : 0u;
        const uint32_t vc[1] = {(anchor && !cvs) ? (uint32_t)d : 0u};
        uint32_t incC[1], exC[1];
        ScanMsb::block(vc, (anchor && cvs) ? 1u : 0u, incC, exC, seg, hseg);
    }
    const uint32_t vn[2] = {cvs_count, 0u};
    uint32_t incN[2], exN[2], tot[2] = {0, 0}, htot = 0;
    Scan<2, 0u, 0u, 0u>::block(vn, 0, incN, exN, tot, htot);
    if (threadIdx.x == 0) {
        uint32_t* p = a.part3 + (uint64_t)blockIdx.x * 8;
        p[0] = tot[0]; p[1] = seg[0]; p[2] = 0; p[3] = 0; p[4] = 0; p[5] = 0; p[6] = 0; p[7] = hseg;
    }
}

__global__ __launch_bounds__(kT) void k_au_scan3(AuArgs a, uint64_t blocks)
{
    uint32_t run[2] = {0u, (a.initial.flags & 2u) ? (uint32_t)a.initial.anchor_poc_msb : 0u}, hrun = 0;
    if (blocks) ScanPart3::parts(a.part3, blocks, run, hrun);
    if (threadIdx.x != 0) return;
    const uint32_t err = blocks ? a.ctl[0] : 0u, aus = blocks ? a.ctl[1] : 0u, pics = blocks ? a.ctl[2] : 0u;
    hbs_summary sm;
    sm.nal_count = aus; sm.nal_found = a.n_nals; sm.rbsp_bytes = 0;
    sm.stream_bytes = a.n_nals ? a.digest[a.n_nals - 1].end : 0;
    sm.stop_reason = 0; sm.error = (int32_t)err;
    sm.reserved[0] = pics; sm.reserved[1] = run[0]; sm.reserved[2] = 0;
    *a.summary = sm;
    if (!blocks) a.ctl[0] = 0;
    if (a.carry_out && a.au && !err) {
        hbs_au_carry c = a.initial;
        c.reserved = 0;
        if (blocks) {
            const uint32_t last_pic = a.ctl[3], last_anchor = a.ctl[4], last_eos = a.ctl[5];
            const bool eos_pending = last_pic ? last_eos > last_pic : (last_eos != 0 || (a.initial.flags & 4u));
            c.flags = (a.initial.flags & 3u) | (last_pic ? 1u : 0u) | (last_anchor ? 2u : 0u) | (eos_pending ? 4u : 0u);
            if (last_anchor) c.anchor_poc_lsb = a.digest[last_anchor - 1].lsb;
            c.anchor_poc_msb = (c.flags & 2u) ? (int32_t)run[1] : 0;
            if (!(c.flags & 2u)) c.anchor_poc_lsb = 0;
        }
        *a.carry_out = c;
    }
}

__global__ __launch_bounds__(kT) void k_au_write(AuArgs a)
{
    if (a.ctl[0] != 0) return;
    const uint64_t base = (uint64_t)blockIdx.x * kAuNalsPerBlock;
    const uint32_t* p2 = a.part2 + (uint64_t)blockIdx.x * 8;
    uint32_t runS[2] = {p2[0], p2[2]}, hS = 0;
    uint32_t runC[1] = {a.part3[(uint64_t)blockIdx.x * 8 + 1]}, hC = 0;
    uint32_t runD[5] = {0, 0, 0, 0, 0}, hD = 0;
    uint32_t* lead = a.lead + (uint64_t)blockIdx.x * 8;
    for (int s = 0; s < kSteps; ++s) {
        const uint64_t k = base + (uint64_t)s * kT + threadIdx.x;
        const bool valid = k < a.n_nals;
        AuDigest g;
        g.cls = 0; g.lsb = 0; g.end = 0;
        if (valid) g = load_digest(a.digest, k);
        const uint32_t cls = g.cls, k1 = (uint32_t)k + 1u;
        const bool start = cls & AU_C_START, pic = cls & AU_C_PIC, cvs = cls & AU_C_CVS;
        const uint32_t pflags = pic ? au_picture_flags(cls) : 0u;
        const bool anchor = pflags & HBS_AU_ANCHOR;
        const uint32_t dsign = (cls >> AU_C_DSIGN_SHIFT) & 3u, mx = 16u << ((cls >> AU_C_DLOG_SHIFT) & 15u);
        const uint32_t d = dsign == 1u ? mx : dsign == 2u ? 0u - mx : 0u;
        const uint32_t vs[2] = {start ? 1u : 0u, start ? k1 : 0u};
        uint32_t incS[2], exS[2];
        ScanStart::block(vs, 0, incS, exS, runS, hS);
        const uint32_t vc[1] = {(anchor && !cvs) ? d : 0u};
        uint32_t incC[1], exC[1];
        ScanMsb::block(vc, (anchor && cvs) ? 1u : 0u, incC, exC, runC, hC);
        const uint32_t poc = pic ? (cvs ? 0u : exC[0] + d) + (uint32_t)g.lsb : 0u;
        const int t = au_type(cls);
        uint32_t bits = 0;
        if (valid) {
            if (cls & AU_C_DAMAGED) bits |= HBS_AU_DAMAGED;
            if (t >= 32 && t <= 34) bits |= HBS_AU_PARAM_SETS;
            if (t == 36 || t == 37) bits |= HBS_AU_END_OF_SEQ;
            if (pic) bits |= pflags | (cvs ? (uint32_t)HBS_AU_CVS_START : 0u);
            const uint32_t st = (cls >> AU_C_STYPE_SHIFT) & 3u;
            if (au_is_vcl(cls) && (cls & AU_C_INDEP) && st < 3u) bits |= 256u << st;
        }
        const uint32_t vd[5] = {valid ? 1u : 0u, (valid && au_is_vcl(cls)) ? 1u : 0u, bits, pic ? k1 : 0u, poc};
        uint32_t incD[5], exD[5];
        ScanAu::block(vd, start ? 1u : 0u, incD, exD, runD, hD);
        if (!valid) continue;
        const uint32_t au = incS[0] - 1u;
        if (a.nal_au) a.nal_au[k] = au;
        if (s == 0 && threadIdx.x == 0 && start) lead[0] = 0;
        const bool closes = k + 1 == a.n_nals || (a.digest[k + 1].cls & AU_C_START);      /* the AU's last NAL */
        if (!(closes || k + 1 == base + kAuNalsPerBlock)) continue;
        const uint64_t first = (uint64_t)incS[1] - 1;
        if (first < base) {               /* the AU began in an earlier workgroup: this one's share (k_au_fix) */
            lead[0] = incD[0]; lead[1] = incD[1]; lead[2] = incD[2]; lead[3] = incD[3]; lead[4] = incD[4];
            lead[5] = closes ? 1u : 0u; lead[6] = (uint32_t)g.end; lead[7] = (uint32_t)(g.end >> 32);
            continue;
        }
        hbs_access_unit r;
        r.first_nal = first;
        r.unit_begin = first ? a.digest[first - 1].end : 0;
        r.unit_end = g.end;
        r.nal_count = incD[0]; r.vcl_count = incD[1];
        r.slice_types = (incD[2] >> 8) & 7u;
        r.flags = incD[2] & 0xFFu;
        r.reserved = 0;
        if (incD[3]) {
            const AuDigest pg = load_digest(a.digest, incD[3] - 1);
            r.first_vcl = (uint32_t)((uint64_t)(incD[3] - 1) - first);
            r.nal_unit_type = au_type(pg.cls); r.temporal_id_plus1 = au_tid1(pg.cls);
            r.pic_order_cnt = (int32_t)incD[4]; r.poc_lsb = pg.lsb;
        } else {
            r.first_vcl = ~0u; r.nal_unit_type = -1; r.temporal_id_plus1 = 0; r.pic_order_cnt = 0; r.poc_lsb = 0;
            r.flags |= HBS_AU_NO_PICTURE;
        }
        a.au[au] = r;
    }
}

__global__ __launch_bounds__(256) void k_au_fix(AuArgs a, uint64_t blocks)
{
    if (a.ctl[0] != 0) return;
    const uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x + 1;
    if (b >= blocks) return;
    const uint32_t* lead = a.lead + b * 8;
    if (lead[0] == 0) return;
    hbs_access_unit* r = a.au + (a.part2[b * 8] - 1u);
    atomicAdd(&r->nal_count, lead[0]);
    atomicAdd(&r->vcl_count, lead[1]);
    if ((lead[2] >> 8) & 7u) atomicOr(&r->slice_types, (lead[2] >> 8) & 7u);
    if (lead[3]) {                                   /* the AU's picture NAL lies in this workgroup: nobody else writes these */
        const AuDigest pg = load_digest(a.digest, lead[3] - 1);
        r->first_vcl = (uint32_t)((uint64_t)(lead[3] - 1) - r->first_nal);
        r->nal_unit_type = au_type(pg.cls); r->temporal_id_plus1 = au_tid1(pg.cls);
        r->pic_order_cnt = (int32_t)lead[4]; r->poc_lsb = pg.lsb;
        atomicAnd(&r->flags, ~(uint32_t)HBS_AU_NO_PICTURE);
    }
    if (lead[2] & 0xFFu) atomicOr(&r->flags, lead[2] & 0xFFu);
    if (lead[5]) r->unit_end = (uint64_t)lead[6] | ((uint64_t)lead[7] << 32);
}

/* ---- hbs_au_keep ---- */
__global__ __launch_bounds__(256) void k_aukeep_sets(AuKeepArgs a)
{
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= a.n_nals) return;
    const uint64_t au = a.nal_au[k];
    if (au >= a.first_au) {
        if (au - a.first_au < a.au_count && (k == 0 || a.nal_au[k - 1] < a.first_au)) a.sets[3] = 1;     /* the range is not empty */
        return;
    }
    const hbs_parsed_nal p = a.parsed[k];
    if (p.rc >= 0 && p.nal_unit_type >= 32 && p.nal_unit_type <= 34) atomicMax(&a.sets[p.nal_unit_type - 32], (uint32_t)k + 1u);
}

__global__ __launch_bounds__(256) void k_aukeep_mask(AuKeepArgs a)
{
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= a.n_nals) return;
    const uint64_t au = a.nal_au[k];
    bool keep = au >= a.first_au && au - a.first_au < a.au_count;
    if ((a.flags & HBS_AUKEEP_PARAM_SETS) && a.sets[3]) {
        const uint32_t k1 = (uint32_t)k + 1u;
        keep = keep || a.sets[0] == k1 || a.sets[1] == k1 || a.sets[2] == k1;
    }
    a.keep[k] = keep ? 1 : 0;
}

} // namespace

hipError_t launch_access_units(const AuArgs& a, hipStream_t st)
{
    const uint64_t blocks = (a.n_nals + kAuNalsPerBlock - 1) / kAuNalsPerBlock;
    const hipError_t e = begin_launches(a.ev_begin, st);
    if (e != hipSuccess) return e;
    if (blocks) {
        hipLaunchKernelGGL(k_au_digest, dim3((unsigned)blocks), dim3(kT), 0, st, a);
        hipLaunchKernelGGL(k_au_scan1, dim3(1), dim3(kT), 0, st, a, blocks);
        hipLaunchKernelGGL(k_au_group, dim3((unsigned)blocks), dim3(kT), 0, st, a);
        hipLaunchKernelGGL(k_au_scan2, dim3(1), dim3(kT), 0, st, a, blocks);
        hipLaunchKernelGGL(k_au_poc, dim3((unsigned)blocks), dim3(kT), 0, st, a);
    }
    hipLaunchKernelGGL(k_au_scan3, dim3(1), dim3(kT), 0, st, a, blocks);
    if (blocks && a.au) {
        hipLaunchKernelGGL(k_au_write, dim3((unsigned)blocks), dim3(kT), 0, st, a);
        if (blocks > 1) hipLaunchKernelGGL(k_au_fix, dim3((unsigned)((blocks - 1 + 255) / 256)), dim3(256), 0, st, a, blocks);
    }
    return end_launches(a.ev_end, st);
}

hipError_t launch_au_keep(const AuKeepArgs& a, hipStream_t st)
{
    hipError_t e = clear_async(a.sets, 16, st);
    if (e != hipSuccess) return e;
    if (a.n_nals) {
        const unsigned g = (unsigned)((a.n_nals + 255) / 256);
        hipLaunchKernelGGL(k_aukeep_sets, dim3(g), dim3(256), 0, st, a);
        hipLaunchKernelGGL(k_aukeep_mask, dim3(g), dim3(256), 0, st, a);
    }
    return hipGetLastError();
}

} // namespace hbs
