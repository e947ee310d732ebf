/*
 * hbs_rtpord.h -- hbs_rtp_order (include/hevcbitstream_amd.h): the rule of the jitter-buffer step as host/device inline
 * functions -- rtpo_params_ok refuses what the call refuses, rtpo_read classes a packet (on top of rtp_packet_rule, hbs_rtp.h),
 * rtpo_sext16 / rtpo_first_ext / rtpo_step make the extended sequence numbers, rtpo_late and rtpo_span say what is late and
 * how wide the kept range is; the kernels of hbs_rtpord.hip and the tests run them -- and the host-visible launcher.
 * Everything above the launcher compiles with plain g++.
 */
#ifndef HBS_RTPORD_H
#define HBS_RTPORD_H

#include "hbs_rtp.h"

namespace hbs {

constexpr int kRtpoLanes = 256;                      /* a lane a packet, or a lane a slot: 256 a workgroup              */
constexpr uint32_t kRtpoFlags = HBS_RTPO_MATCH_SSRC | HBS_RTPO_AFTER;
constexpr uint64_t kRtpoMaxPackets = 0xFFFFFFFEull;  /* a table position fits a slot, and 0xFFFFFFFF is left for "empty" */
constexpr uint64_t kRtpoMaxSpan = 1ull << 33;
constexpr uint64_t kRtpoExtStart = 1ull << 48;       /* ext of the first accepted packet = this + its seq                */
constexpr uint64_t kRtpoAfterMin = 1ull << 48, kRtpoAfterMax = 1ull << 62;
constexpr uint32_t kRtpoEmpty = 0xFFFFFFFFu;         /* a slot no packet has taken                                       */
constexpr uint64_t kRtpoSlotGridMax = 16384;         /* workgroups of a launch over the slots; each loops to the span    */

/* the classes of a packet, in the order of the rule */
enum : uint32_t { kRtpoFault = 0, kRtpoOther = 1, kRtpoAccepted = 2 };

/* what of hbs_rtp_order_params the rule reads */
struct RtpoRule {
    uint32_t pt, ssrc;
    uint32_t match_ssrc, after;
    uint64_t max_span, after_ext;
};

struct RtpoPacket {
    uint32_t cls, seq;
};

HBS_HD bool rtpo_params_ok(const hbs_rtp_order_params* p)
{
    if (!p || p->payload_type < 0 || p->payload_type > 127) return false;
    if ((p->flags & ~kRtpoFlags) != 0u || p->reserved != 0u) return false;
    if (p->max_span < 1 || p->max_span > kRtpoMaxSpan) return false;
    return !(p->flags & HBS_RTPO_AFTER) || (p->after_ext >= kRtpoAfterMin && p->after_ext <= kRtpoAfterMax);
}

HBS_HD RtpoRule rtpo_rule(const hbs_rtp_order_params* p)
{
    RtpoRule q;
    q.pt = (uint32_t)p->payload_type; q.ssrc = p->ssrc;
    q.match_ssrc = (p->flags & HBS_RTPO_MATCH_SSRC) ? 1u : 0u; q.after = (p->flags & HBS_RTPO_AFTER) ? 1u : 0u;
    q.max_span = p->max_span; q.after_ext = q.after ? p->after_ext : 0;
    return q;
}

/* the packet of n bytes whose byte i is byte(i): steps 1 (its header part) and 2 of the rule */
template <class B> HBS_HD RtpoPacket rtpo_read(B byte, uint64_t n, const RtpoRule& q)
{
    RtpoPacket r;
    r.cls = kRtpoFault; r.seq = 0;
    hbs_rtp_packet k;
    if (rtp_packet_rule(byte, n, &k) != 0) return r;
    r.seq = k.seq;
    r.cls = (k.payload_type != q.pt || (q.match_ssrc && k.ssrc != q.ssrc)) ? kRtpoOther : kRtpoAccepted;
    return r;
}

/* the low 16 bits of x read as a signed number, as a two's-complement 64-bit word */
HBS_HD uint64_t rtpo_sext16(uint64_t x) { return ((x & 0xFFFFull) ^ 0x8000ull) - 0x8000ull; }

/* ext of the first accepted packet of the table */
HBS_HD uint64_t rtpo_first_ext(const RtpoRule& q, uint32_t seq)
{
    return q.after ? q.after_ext + rtpo_sext16((uint64_t)seq - q.after_ext) : kRtpoExtStart + seq;
}

/* ext(a_i) - ext(a_(i-1)), as a two's-complement 64-bit word */
HBS_HD uint64_t rtpo_step(uint32_t prev_seq, uint32_t seq) { return rtpo_sext16((uint64_t)seq - (uint64_t)prev_seq); }

HBS_HD bool rtpo_late(const RtpoRule& q, uint64_t ext) { return q.after && ext <= q.after_ext; }

/* where the slots begin, given the lowest ext that is not late */
HBS_HD uint64_t rtpo_base(const RtpoRule& q, uint64_t lowest) { return q.after ? q.after_ext + 1u : lowest; }

/* the span of `live` accepted packets that are not late, the lowest and the highest of them given */
HBS_HD uint64_t rtpo_span(const RtpoRule& q, uint64_t live, uint64_t lowest, uint64_t highest)
{
    return live ? highest - rtpo_base(q, lowest) + 1u : 0u;
}

/* workgroups for n packets, or n slots */
HBS_HD uint64_t rtpo_blocks(uint64_t n) { return (n + kRtpoLanes - 1) / kRtpoLanes; }

#ifdef __HIPCC__
} // namespace hbs
#include <hip/hip_runtime_api.h>
namespace hbs {

struct RtpoArgs {
    const uint8_t* src; uint64_t n;                   /* the input                                                      */
    const unsigned long long* pkt_off; const unsigned long long* pkt_size; uint64_t n_packets;
    RtpoRule q;
    unsigned long long* off_out; unsigned long long* size_out;       /* both or neither (plan only)                    */
    uint32_t* src_out; unsigned long long* ext_out;                  /* nullable                                       */
    uint64_t out_cap;
    hbs_summary* summary;
    /* scratch (lay_rtpo) */
    uint32_t* rec;                  /* n_packets: seq | accepted << 16 | accepted and not late << 17                  */
    unsigned long long* ext;        /* n_packets, written and read for accepted packets only: the sum of the differences inside
                                       the workgroup, then ext                                                       */
    unsigned long long* part_a;     /* 8 per block: accepted packets, 1 + the lowest faulty entry                     */
    unsigned long long* part_d;     /* 8 per block: the sum of the block's differences, 0                             */
    unsigned long long* last_a;     /* 1 per block: (1 + the last accepted packet) << 16 | its seq, then of the blocks in front */
    unsigned long long* last_m;     /* 1 per block: the highest ext that is not late, then of the blocks in front     */
    unsigned long long* low_m;      /* 2 per block: ~(the lowest ext that is not late) (0: none), their number         */
    unsigned long long* moved_m;    /* 1 per block: kept packets that have moved                                      */
    uint32_t* slot;                 /* max_span: the first table position that carries ext = base + i, or kRtpoEmpty   */
    unsigned long long* part_s;     /* 8 per 256 slots: taken slots, 0                                                */
    unsigned long long* ctl;        /* 16: 0 error, 1 accepted, 2 the highest ext that is not late, 3 accepted and not late,
                                       4 base, 5 span                                                                */
    uint64_t slot_grid;             /* workgroups of a launch over the slots                                          */
    hipEvent_t ev_begin, ev_end;
};

/* the scratch the call needs, sized by a.n_packets and a.q.max_span */
inline void lay_rtpo(Carver& w, RtpoArgs& a)
{
    const uint64_t blocks = rtpo_blocks(a.n_packets), sblocks = rtpo_blocks(a.q.max_span);
    a.rec = w.take<uint32_t>(a.n_packets * 4);
    a.ext = w.take<unsigned long long>(a.n_packets * 8);
    a.part_a = w.take<unsigned long long>(blocks * 64);
    a.part_d = w.take<unsigned long long>(blocks * 64);
    a.last_a = w.take<unsigned long long>(blocks * 8);
    a.last_m = w.take<unsigned long long>(blocks * 8);
    a.low_m = w.take<unsigned long long>(blocks * 16);
    a.moved_m = w.take<unsigned long long>(blocks * 8);
    a.slot = w.take<uint32_t>(a.q.max_span * 4);
    a.part_s = w.take<unsigned long long>(sblocks * 64);
    a.ctl = w.take<unsigned long long>(128);
    a.slot_grid = sblocks < kRtpoSlotGridMax ? sblocks : kRtpoSlotGridMax;
}
hipError_t launch_rtp_order(const RtpoArgs& a, hipStream_t st);
#endif

} // namespace hbs
#endif
