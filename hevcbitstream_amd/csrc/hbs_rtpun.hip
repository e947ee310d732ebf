/*
 * hbs_rtpun.hip -- hbs_rtp_unpack: RTP packets by RFC 7798 -> the Annex-B stream of their NAL units, single NAL unit packets,
 * aggregation packets and fragmentation units (include/hevcbitstream_amd.h is the specification; the packet rule is rtpu_read /
 * rtpu_ap_walk / rtpu_continues, hbs_rtpun.h).  A lane a packet, 256 packets a workgroup; a plan of eight launches that ends in
 * a table of pieces with a literal each, and the copy over it (hbs_pieces.h).  No launch waits for another workgroup:
 *
 *   k_rtpu_class   checks the table entry, then the packet's header (its first 16 bytes from one or two aligned 16-byte loads,
 *                  which covers the header, the PayloadHdr and the FU header of a packet without CSRC entries; more bytes are
 *                  read one by one), walks an aggregation packet's units, reads the header of the packet in front once more for
 *                  "continues"; leaves a record a packet, and per workgroup the chains begun and 1 + its lowest faulty packet
 *   k_rtpu_scan_c  one workgroup: the chains in front of each workgroup (scan_parts, hbs_plan.h); on a fault the error and the
 *                  summary, and every later launch returns at once
 *   k_rtpu_chain   every FU its chain's number; the chain's first packet leaves "has S", its last "has E" in the chain's record
 *   k_rtpu_count   every FU asks its chain's record whether the chain is whole; per packet its output bytes, NALs, pieces,
 *                  whether it is dropped, whether it and the packet in front of it break the sequence; a whole chain's NAL counts
 *                  at its last packet, which also carries the chain's marker.  Per workgroup the sums and 1 + the last packet
 *                  that gives NALs
 *   k_rtpu_scan_n  one workgroup: the sums become offsets, and "the last packet that gives NALs" becomes what lies in front of
 *                  each workgroup (an exclusive max-scan)
 *   k_rtpu_au      a packet that gives NALs finds the last such packet in front of it (the max-scan inside the workgroup and the
 *                  one over the workgroups) and reads its timestamp and marker: does its first NAL begin an access unit?
 *   k_rtpu_scan_a  one workgroup: the access units in front of each workgroup; the totals, the capacities, the summary.  A
 *                  plan-only call ends here
 *   k_rtpu_place   the packets once more, now with the offsets: the piece table, d_index_out (a chain's start by the lane of
 *                  its first packet, its end by the lane of its last), d_nal_au_out, d_au_ts_out
 *   copy_pieces    (hbs_pieces.hip) with a literal a piece
 *
 * Traffic: the payloads read once and written once; per packet 16 B of the table three times, its header granules twice, 20 B of
 * scratch written and read two to four times, 24 B a piece; per NAL 36 B of output tables.
 */
#include <hip/hip_runtime.h>
#include "hbs_rtpun.h"
#include "hbs_plan.h"
#include "hbs_rtpbytes.h"

namespace hbs {
namespace {

constexpr int kT = kPlanLanes;
static_assert(kRtpuPacketsPerBlock == kT, "one packet a lane");

enum : uint32_t { kBitS = 1u << 3, kBitE = 1u << 4, kBitCont = 1u << 5, kBitMarker = 1u << 6 };
enum : uint32_t { kWhole = 1u, kGives = 2u, kLast = 4u, kAuStart = 8u };

__device__ __forceinline__ uint32_t rec_class(uint32_t bits) { return bits & 7u; }
__device__ __forceinline__ uint32_t rec_pad(uint32_t bits) { return (bits >> 8) & 0xFFu; }
__device__ __forceinline__ uint32_t rec_seq(uint32_t bits) { return bits >> 16; }

/* table entry p: checked before a byte of the packet is read */
__device__ __forceinline__ RtpuPacket read_entry(const RtpuArgs& a, uint64_t p, PacketBytes& pb, uint64_t& size)
{
    const uint64_t off = a.pkt_off[p];
    size = a.pkt_size[p];
    RtpuPacket r;
    r.cls = kRtpuFault; r.marker = r.seq = r.ts = r.ssrc = 0; r.fu_s = r.fu_e = r.fu_type = 0; r.h0 = r.h1 = 0;
    r.pay_off = r.pay_len = 0; r.pad = 0;
    pb.p = a.t.src; pb.lo = pb.hi = 0;
    if (size > a.n || off > a.n - size || size < kRtpHeader) return r;
    pb = load_packet(a.t.src, off, size);
    return rtpu_read(pb, size, a.q);
}

__global__ __launch_bounds__(kT) void k_rtpu_class(RtpuArgs a)
{
    const uint64_t p = (uint64_t)blockIdx.x * kT + threadIdx.x;
    uint64_t v[1] = {0};
    uint64_t bad = 0;
    if (p < a.n_packets) {
        PacketBytes pb;
        uint64_t size;
        RtpuPacket x = read_entry(a, p, pb, size);
        bool cont = false;
        if (x.cls == kRtpuFu && !x.fu_s && p) {
            PacketBytes qb;
            uint64_t qsize;
            const RtpuPacket y = read_entry(a, p - 1, qb, qsize);
            cont = rtpu_continues(x, y);
        }
        if (x.cls == kRtpuAp) {
            uint64_t units, bytes;
            if (!rtpu_ap_walk(pb, x.pay_off, x.pay_len, units, bytes, [](uint64_t, uint64_t) {})) x.cls = kRtpuFault;
            a.ap[2 * p] = units; a.ap[2 * p + 1] = bytes;
        }
        if (x.cls == kRtpuFault) bad = p + 1;
        if (x.cls == kRtpuFu && !cont) v[0] = 1;
        RtpuRec r;
        r.bits = x.cls | (x.fu_s ? kBitS : 0u) | (x.fu_e ? kBitE : 0u) | (cont ? kBitCont : 0u) | (x.marker ? kBitMarker : 0u) | (x.pad << 8) | (x.seq << 16);
        r.ts = x.ts; r.pay_off = (uint32_t)x.pay_off; r.chain = 0;
        a.rec[p] = r;
    }
    bad = block_min_nonzero(bad);
    uint64_t ex[1], tot[1];
    block_scan<1, kT>(v, ex, tot);
    if (threadIdx.x == 0) {
        unsigned long long* q = a.part_c + (uint64_t)blockIdx.x * 8;
        q[0] = tot[0]; q[1] = bad;
    }
}

__global__ __launch_bounds__(kT) void k_rtpu_scan_c(RtpuArgs a, uint64_t blocks)
{
    uint64_t carry[1];
    const uint64_t bad = scan_parts<1>(a.part_c, blocks, carry);
    if (threadIdx.x != 0) return;
    a.t.ctl[0] = bad ? (unsigned long long)(uint32_t)HBS_E_ARG : 0ull;
    a.t.ctl[1] = 0; a.t.ctl[2] = 0; a.t.ctl[3] = carry[0];
    if (bad) {
        hbs_summary s;
        s.nal_count = 0; s.nal_found = 0; s.rbsp_bytes = 0; s.stream_bytes = 0;
        s.stop_reason = 0; s.error = HBS_E_ARG;
        s.reserved[0] = bad; s.reserved[1] = s.reserved[2] = 0;
        *a.summary = s;
    }
}

/* is packet p the last of its chain?  (p an FU) */
__device__ __forceinline__ bool chain_ends_at(const RtpuArgs& a, uint64_t p)
{
    if (p + 1 == a.n_packets) return true;
    const uint32_t next = a.rec[p + 1].bits;
    return !(rec_class(next) == kRtpuFu && (next & kBitCont));
}

__global__ __launch_bounds__(kT) void k_rtpu_chain(RtpuArgs a)
{
    if (a.t.ctl[0] != 0) return;
    const uint64_t p = (uint64_t)blockIdx.x * kT + threadIdx.x;
    const bool in = p < a.n_packets;
    const uint32_t bits = in ? a.rec[p].bits : 0u;
    const bool fu = rec_class(bits) == kRtpuFu, begins = fu && !(bits & kBitCont);
    uint64_t v[1] = {begins ? 1u : 0u};
    uint64_t ex[1], tot[1];
    block_scan<1, kT>(v, ex, tot);
    if (!fu) return;
    const uint64_t c = a.part_c[(uint64_t)blockIdx.x * 8] + ex[0] + v[0] - 1;        /* (an FU continues, or begins a chain) */
    a.rec[p].chain = (uint32_t)c;
    if (begins) a.chain_w[2 * c] = (bits & kBitS) ? 1u : 0u;
    if (chain_ends_at(a, p)) a.chain_w[2 * c + 1] = (bits & kBitE) ? 1u : 0u;
}

/* what packet p gives, once the chains are known */
struct Gives {
    uint64_t out, nals, pieces;
    uint32_t state;
    bool dropped;
};

__device__ __forceinline__ Gives gives(const RtpuArgs& a, uint64_t p, const RtpuRec& r)
{
    Gives g;
    g.out = g.nals = g.pieces = 0; g.state = 0; g.dropped = false;
    const uint32_t cls = rec_class(r.bits);
    const uint64_t pay_len = a.pkt_size[p] - r.pay_off - rec_pad(r.bits);
    if (cls == kRtpuSingle) {
        g.out = a.q.sc + pay_len; g.nals = 1; g.pieces = 1; g.state = kGives;
    } else if (cls == kRtpuAp) {
        const uint64_t units = a.ap[2 * p], bytes = a.ap[2 * p + 1];
        g.out = a.q.sc * units + bytes; g.nals = units; g.pieces = units; g.state = kGives;
    } else if (cls == kRtpuFu) {
        if (a.chain_w[2 * (uint64_t)r.chain] && a.chain_w[2 * (uint64_t)r.chain + 1]) {
            const bool last = chain_ends_at(a, p);
            g.out = pay_len - kRtpFuHeader + ((r.bits & kBitCont) ? 0u : a.q.sc + 2u);
            g.nals = last ? 1 : 0; g.pieces = 1;
            g.state = kWhole | (last ? kGives | kLast : 0u);
        } else {
            g.dropped = true;
        }
    } else if (cls == kRtpuUnsupported) {
        g.dropped = true;
    }
    return g;
}

__global__ __launch_bounds__(kT) void k_rtpu_count(RtpuArgs a)
{
    if (a.t.ctl[0] != 0) return;
    const uint64_t p = (uint64_t)blockIdx.x * kT + threadIdx.x;
    uint64_t v[5] = {0, 0, 0, 0, 0};
    uint64_t gives_at = 0;
    if (p < a.n_packets) {
        const RtpuRec r = a.rec[p];
        const Gives g = gives(a, p, r);
        a.state[p] = g.state;
        v[0] = g.out; v[1] = g.nals; v[2] = g.pieces; v[3] = g.dropped ? 1 : 0;
        if (rtpu_accepted(rec_class(r.bits))) {
            v[4] = 1;
            if (p) {
                const uint32_t prev = a.rec[p - 1].bits;
                if (rtpu_accepted(rec_class(prev)) && rec_seq(r.bits) != ((rec_seq(prev) + 1u) & 0xFFFFu)) v[3] += 1ull << 32;
            }
        }
        if (g.state & kGives) gives_at = p + 1;
    }
    uint64_t ex[5], tot[5];
    block_scan<5, kT>(v, ex, tot);
    uint64_t mex, mtot;
    block_excl_max<uint64_t, 1, kT>(&gives_at, &mex, &mtot);
    if (threadIdx.x == 0) {
        unsigned long long* q = a.part_n + (uint64_t)blockIdx.x * 8;
        q[0] = tot[0]; q[1] = tot[1]; q[2] = tot[2]; q[3] = tot[3]; q[4] = tot[4]; q[5] = 0;
        a.last_n[blockIdx.x] = mtot;
    }
}

__global__ __launch_bounds__(kT) void k_rtpu_scan_n(RtpuArgs a, uint64_t blocks)
{
    if (a.t.ctl[0] != 0) return;
    uint64_t carry[5];
    (void)scan_parts<5>(a.part_n, blocks, carry);
    uint64_t run = 0;
    for (uint64_t seg = 0; seg < blocks; seg += (uint64_t)kT * kPlanPer) {
        const uint64_t i0 = seg + (uint64_t)threadIdx.x * kPlanPer;
        uint64_t acc = 0;
        for (int i = 0; i < kPlanPer && i0 + i < blocks; ++i) { const uint64_t x = a.last_n[i0 + i]; if (x > acc) acc = x; }
        uint64_t cur, tot;
        block_excl_max<uint64_t, 1, kT>(&acc, &cur, &tot);
        if (run > cur) cur = run;
        for (int i = 0; i < kPlanPer && i0 + i < blocks; ++i) {
            const uint64_t x = a.last_n[i0 + i];
            a.last_n[i0 + i] = cur;
            if (x > cur) cur = x;
        }
        if (tot > run) run = tot;
    }
    if (threadIdx.x == 0) { a.t.ctl[1] = carry[0]; a.t.ctl[2] = carry[2]; a.t.ctl[4] = carry[1]; a.t.ctl[5] = carry[3]; a.t.ctl[6] = carry[4]; }
}

__global__ __launch_bounds__(kT) void k_rtpu_au(RtpuArgs a)
{
    if (a.t.ctl[0] != 0) return;
    const uint64_t p = (uint64_t)blockIdx.x * kT + threadIdx.x;
    const bool in = p < a.n_packets;
    const uint32_t st = in ? a.state[p] : 0u;
    const bool gives_nals = (st & kGives) != 0;
    const uint64_t gives_at = gives_nals ? p + 1 : 0;
    uint64_t before, all;
    block_excl_max<uint64_t, 1, kT>(&gives_at, &before, &all);
    uint64_t v[1] = {0};
    if (gives_nals) {
        const uint64_t far = a.last_n[blockIdx.x];
        if (far > before) before = far;
        if (before == 0) v[0] = 1;
        else {
            const RtpuRec prev = a.rec[before - 1], cur = a.rec[p];
            v[0] = (prev.ts != cur.ts || (prev.bits & kBitMarker)) ? 1 : 0;
        }
        if (v[0]) a.state[p] = st | kAuStart;
    }
    uint64_t ex[1], tot[1];
    block_scan<1, kT>(v, ex, tot);
    if (threadIdx.x == 0) {
        unsigned long long* q = a.part_a + (uint64_t)blockIdx.x * 8;
        q[0] = tot[0]; q[1] = 0;
    }
}

__global__ __launch_bounds__(kT) void k_rtpu_scan_a(RtpuArgs a, uint64_t blocks)
{
    if (a.t.ctl[0] != 0) return;
    uint64_t carry[1];
    (void)scan_parts<1>(a.part_a, blocks, carry);
    if (threadIdx.x != 0) return;
    const uint64_t total = a.t.ctl[1], pieces = a.t.ctl[2], nals = a.t.ctl[4], aus = carry[0];
    const bool over = a.t.out && (total > a.out_cap || nals > a.nal_cap || (a.au_ts_out && aus > a.au_cap));
    const int32_t err = over ? HBS_E_CAPACITY : 0;
    a.t.ctl[0] = (unsigned long long)(uint32_t)err;
    if (!err && a.t.out) a.t.piece_out[pieces] = total;
    hbs_summary s;
    s.nal_count = nals; s.nal_found = a.t.ctl[6]; s.rbsp_bytes = total - nals * a.q.sc; s.stream_bytes = total;
    s.stop_reason = nals ? -1 : 0; s.error = err;
    s.reserved[0] = 0; s.reserved[1] = aus; s.reserved[2] = a.t.ctl[5];
    *a.summary = s;
}

__global__ __launch_bounds__(kT) void k_rtpu_place(RtpuArgs a)
{
    if (a.t.ctl[0] != 0) return;
    const uint64_t p = (uint64_t)blockIdx.x * kT + threadIdx.x;
    const bool in = p < a.n_packets;
    uint64_t v[4] = {0, 0, 0, 0};
    RtpuRec r;
    r.bits = 0; r.ts = 0; r.pay_off = 0; r.chain = 0;
    uint32_t st = 0;
    if (in) {
        r = a.rec[p];
        st = a.state[p];
        const Gives g = gives(a, p, r);
        v[0] = g.out; v[1] = g.nals; v[2] = g.pieces; v[3] = (st & kAuStart) ? 1 : 0;
    }
    uint64_t off[4], tot[4];
    block_scan<4, kT>(v, off, tot);
    if (!in || !v[2]) return;
    const unsigned long long* part = a.part_n + (uint64_t)blockIdx.x * 8;
    uint64_t o = off[0] + part[0], k = off[1] + part[1], j = off[2] + part[2];
    const uint64_t au = off[3] + a.part_a[(uint64_t)blockIdx.x * 8] + v[3] - 1;       /* read where the packet gives NALs */
    const uint64_t last_nal = a.t.ctl[4] - 1;
    const uint32_t cls = rec_class(r.bits), sc = a.q.sc;
    const uint64_t pkt = a.pkt_off[p], pay = pkt + r.pay_off;
    unsigned long long* const piece_out = a.t.piece_out;
    unsigned long long* const piece_delta = a.t.piece_delta;
    unsigned long long* const piece_lit = a.t.piece_lit;
    hbs_nal_entry* const index_out = a.index_out;
    uint32_t* const nal_au_out = a.nal_au_out;
    /* a NAL of `len` bytes that begins at input byte `src`: the start code, then the bytes */
    auto whole_nal = [&](uint64_t src, uint64_t len) {
        piece_out[j] = o; piece_delta[j] = src - (o + sc); piece_lit[j] = rtpu_literal(sc, false, 0, 0, 0);
        if (index_out) {
            hbs_nal_entry e;
            e.start = o + sc; e.end = o + sc + len; e.rbsp_off = 0; e.rbsp_len = 0; e.status = k == last_nal ? HBS_ST_UNTERMINATED : 0;
            index_out[k] = e;
        }
        if (nal_au_out) nal_au_out[k] = (uint32_t)au;
        o += sc + len; k += 1; j += 1;
    };
    if ((st & kAuStart) && a.au_ts_out) a.au_ts_out[au] = r.ts;
    if (cls == kRtpuSingle) {
        whole_nal(pay, a.pkt_size[p] - r.pay_off - rec_pad(r.bits));
    } else if (cls == kRtpuAp) {
        const uint64_t pay_len = a.pkt_size[p] - r.pay_off - rec_pad(r.bits);
        const uint8_t* const src = a.t.src + pkt;
        uint64_t units, bytes;
        (void)rtpu_ap_walk([src](uint64_t i) -> uint32_t { return src[i]; }, r.pay_off, pay_len, units, bytes,
                           [&](uint64_t at, uint64_t len) { whole_nal(pkt + at, len); });
    } else {                                                         /* an FU of a whole chain */
        const uint64_t frag = a.pkt_size[p] - r.pay_off - rec_pad(r.bits) - kRtpFuHeader;
        const bool first = !(r.bits & kBitCont);
        uint64_t lit = 0;
        if (first) lit = rtpu_literal(sc, true, a.t.src[pay], a.t.src[pay + 2] & 63u, a.t.src[pay + 1]);
        const uint64_t lit_len = lit >> 56;
        piece_out[j] = o; piece_delta[j] = pay + kRtpFuHeader - (o + lit_len); piece_lit[j] = lit;
        if (index_out) {
            if (first) { index_out[k].start = o + sc; index_out[k].rbsp_off = 0; index_out[k].rbsp_len = 0; }
            if (st & kLast) { index_out[k].end = o + lit_len + frag; index_out[k].status = k == last_nal ? HBS_ST_UNTERMINATED : 0; }
        }
        if ((st & kLast) && nal_au_out) nal_au_out[k] = (uint32_t)au;
    }
}

} // namespace

hipError_t launch_rtp_unpack(const RtpuArgs& a, hipStream_t st)
{
    const uint64_t blocks = rtpu_blocks(a.n_packets);
    const dim3 grid((unsigned)blocks), lanes(kT);
    const hipError_t e = begin_launches(a.ev_begin, st);
    if (e != hipSuccess) return e;
    if (blocks) hipLaunchKernelGGL(k_rtpu_class, grid, lanes, 0, st, a);
    hipLaunchKernelGGL(k_rtpu_scan_c, dim3(1), lanes, 0, st, a, blocks);
    if (blocks) {
        hipLaunchKernelGGL(k_rtpu_chain, grid, lanes, 0, st, a);
        hipLaunchKernelGGL(k_rtpu_count, grid, lanes, 0, st, a);
    }
    hipLaunchKernelGGL(k_rtpu_scan_n, dim3(1), lanes, 0, st, a, blocks);
    if (blocks) hipLaunchKernelGGL(k_rtpu_au, grid, lanes, 0, st, a);
    hipLaunchKernelGGL(k_rtpu_scan_a, dim3(1), lanes, 0, st, a, blocks);
    if (a.t.out && blocks) {
        hipLaunchKernelGGL(k_rtpu_place, grid, lanes, 0, st, a);
        (void)copy_pieces(a.t, st);
    }
    return end_launches(a.ev_end, st);
}

} // namespace hbs

extern "C" {

int64_t hbs_rtp_ap_units_host(const uint8_t* pkt, uint64_t n, uint64_t* off_out, uint64_t* size_out, uint64_t cap)
{
    return hbs::rtp_ap_units_host(pkt, n, off_out, size_out, cap);
}

uint64_t hbs_rtp_frames_host(const uint8_t* bytes, uint64_t n, uint64_t* off_out, uint64_t* size_out, uint64_t cap, uint64_t* used_out)
{
    return hbs::rtp_frames_host(bytes, n, off_out, size_out, cap, used_out);
}

}
