/*
 * hbs_rtpun.h -- hbs_rtp_unpack (include/hevcbitstream_amd.h): what the receiver makes of one packet, as host/device inline
 * functions -- rtpu_read classes a packet (on top of rtp_packet_rule, hbs_rtp.h), rtpu_ap_walk walks the units of an
 * aggregation packet, rtpu_continues says whether a fragmentation unit goes on where the packet in front of it stopped; the
 * kernels of hbs_rtpun.hip and the tests run them -- rtp_frames_host (RFC 4571 framing on the host), and the host-visible
 * launcher.  Everything above the launcher compiles with plain g++.
 */
#ifndef HBS_RTPUN_H
#define HBS_RTPUN_H

#include "hbs_rtp.h"
#ifdef __HIPCC__
#include "hbs_pieces.h"
#endif

namespace hbs {

constexpr int kRtpuPacketsPerBlock = 256;           /* a lane a packet, 256 packets a workgroup                       */
constexpr uint32_t kRtpuFlags = HBS_RTPU_MATCH_SSRC;

/* the classes of a packet, in the order of the packet rule */
enum : uint32_t {
    kRtpuFault = 0,                                 /* entry, header, aggregation packet or FU type fault             */
    kRtpuOther = 1,                                 /* not this stream's                                              */
    kRtpuUnsupported = 2,                           /* accepted from here on: no payload header, PACI, reserved types */
    kRtpuSingle = 3,
    kRtpuAp = 4,
    kRtpuFu = 5
};

/* what of hbs_rtp_unpack_params the rule reads */
struct RtpuRule {
    uint32_t pt, ssrc;
    uint32_t match_ssrc;
    uint32_t sc;                                    /* startcode_bytes                                                */
};

struct RtpuPacket {
    uint32_t cls;
    uint32_t marker, seq, ts, ssrc;
    uint32_t fu_s, fu_e, fu_type;                   /* an FU's S, E and type                                          */
    uint32_t h0, h1;                                /* the payload's first two bytes (the PayloadHdr)                 */
    uint64_t pay_off, pay_len;                      /* the payload inside the packet                                  */
    uint32_t pad;                                   /* padding bytes behind it                                        */
};

HBS_HD bool rtpu_accepted(uint32_t cls) { return cls >= kRtpuUnsupported; }

/* the packet of n bytes whose byte i is byte(i): steps 2 to 4 of the packet rule, an aggregation packet's units excepted
 * (rtpu_ap_walk) */
template <class B> HBS_HD RtpuPacket rtpu_read(B byte, uint64_t n, const RtpuRule& q)
{
    RtpuPacket r;
    r.cls = kRtpuFault; r.marker = r.seq = r.ts = r.ssrc = 0; r.fu_s = r.fu_e = r.fu_type = 0; r.h0 = r.h1 = 0;
    r.pay_off = r.pay_len = 0; r.pad = 0;
    hbs_rtp_packet k;
    if (rtp_packet_rule(byte, n, &k) != 0) return r;
    r.marker = k.marker; r.seq = k.seq; r.ts = k.timestamp; r.ssrc = k.ssrc;
    r.pay_off = k.payload_off; r.pay_len = k.payload_len; r.pad = (uint32_t)(n - k.payload_off - k.payload_len);
    if (k.payload_type != q.pt || (q.match_ssrc && k.ssrc != q.ssrc)) { r.cls = kRtpuOther; return r; }
    r.cls = kRtpuUnsupported;
    if (k.kind == HBS_RTP_SINGLE) r.cls = kRtpuSingle;
    else if (k.kind == HBS_RTP_AP) r.cls = kRtpuAp;
    else if (k.kind == HBS_RTP_FU) {
        r.fu_s = k.fu_start; r.fu_e = k.fu_end; r.fu_type = (uint32_t)k.nal_type;
        r.h0 = byte(k.payload_off); r.h1 = k.nal_header[1];
        r.cls = r.fu_type >= 48u ? kRtpuFault : kRtpuFu;
    }
    return r;
}

/* the units of an aggregation packet whose payload is bytes [pay_off, pay_off + pay_len) of the packet: f(where the unit's NAL
 * begins in the packet, its size).  units / bytes: the well-formed units in front of the payload's end or of what is wrong.
 * false: no unit, fewer than 2 bytes left for a size, a size below 2 or beyond what is left, a NAL type of 48 or above.  Every
 * size is bounded before it is used. */
template <class B, class F> HBS_HD bool rtpu_ap_walk(B byte, uint64_t pay_off, uint64_t pay_len, uint64_t& units, uint64_t& bytes, F f)
{
    units = 0; bytes = 0;
    if (pay_len < 2) return false;
    uint64_t p = pay_off + 2;
    const uint64_t e = pay_off + pay_len;
    if (p == e) return false;
    while (p < e) {
        if (e - p < 2) return false;
        const uint64_t s = ((uint64_t)byte(p) << 8) | byte(p + 1);
        p += 2;
        if (s < 2 || s > e - p) return false;
        if (((byte(p) >> 1) & 63u) >= 48u) return false;
        f(p, s);
        p += s; units += 1; bytes += s;
    }
    return true;
}

/* does the accepted FU `cur` continue `prev`, the packet in front of it in the table? */
HBS_HD bool rtpu_continues(const RtpuPacket& cur, const RtpuPacket& prev)
{
    return cur.cls == kRtpuFu && !cur.fu_s && prev.cls == kRtpuFu && !prev.fu_e && cur.fu_type == prev.fu_type &&
           cur.h0 == prev.h0 && cur.h1 == prev.h1 && cur.ts == prev.ts && cur.ssrc == prev.ssrc && cur.seq == ((prev.seq + 1u) & 0xFFFFu);
}

/* the literal in front of a NAL's bytes, as hbs_pieces.h takes it: length << 56, byte i in bits [8 i, 8 i + 8).  fu: the start
 * code and the two header bytes rebuilt from the chain's first packet */
HBS_HD uint64_t rtpu_literal(uint32_t sc, bool fu, uint32_t h0, uint32_t fu_type, uint32_t h1)
{
    const uint64_t one = 1ull << (8u * (sc - 1u));
    if (!fu) return ((uint64_t)sc << 56) | one;
    const uint64_t n0 = (h0 & 0x81u) | (fu_type << 1);
    return ((uint64_t)(sc + 2u) << 56) | one | (n0 << (8u * sc)) | ((uint64_t)h1 << (8u * (sc + 1u)));
}

/* ---- host side ------------------------------------------------------------------------------------------------------------ */

inline bool rtpu_params_ok(const hbs_rtp_unpack_params* p)
{
    if (!p || p->payload_type < 0 || p->payload_type > 127) return false;
    return (p->startcode_bytes == 3 || p->startcode_bytes == 4) && (p->flags & ~kRtpuFlags) == 0u;
}

inline RtpuRule rtpu_rule(const hbs_rtp_unpack_params* p)
{
    RtpuRule q;
    q.pt = (uint32_t)p->payload_type; q.ssrc = p->ssrc; q.match_ssrc = (p->flags & HBS_RTPU_MATCH_SSRC) ? 1u : 0u; q.sc = (uint32_t)p->startcode_bytes;
    return q;
}

/* hbs_rtp_ap_units_host: rtp_packet_rule, then rtpu_ap_walk over the payload */
inline int64_t rtp_ap_units_host(const uint8_t* pkt, uint64_t n, uint64_t* off_out, uint64_t* size_out, uint64_t cap)
{
    hbs_rtp_packet k;
    if (rtp_packet_host(pkt, n, &k) != 0 || k.kind != HBS_RTP_AP) return HBS_E_ARG;
    if (cap && (!off_out || !size_out)) return HBS_E_ARG;
    uint64_t units = 0, bytes = 0, at = 0;
    const bool ok = rtpu_ap_walk(RtpBytesAt{pkt}, k.payload_off, k.payload_len, units, bytes, [&](uint64_t off, uint64_t size) {
        if (at < cap) { off_out[at] = off; size_out[at] = size; }
        ++at;
    });
    return ok ? (int64_t)units : (int64_t)HBS_E_ARG;
}

/* an RFC 4571 byte stream: a 16-bit big-endian length, then a packet of that many bytes, and so on.  Fills up to `cap` offset /
 * size pairs of the packets (the length fields left out), returns the whole frames, *used_out = the bytes they take.  Stops in
 * front of the first incomplete frame; no length is trusted before it is bounded. */
inline uint64_t rtp_frames_host(const uint8_t* bytes, uint64_t n, uint64_t* off_out, uint64_t* size_out, uint64_t cap, uint64_t* used_out)
{
    uint64_t at = 0, frames = 0;
    while (bytes && n - at >= 2) {
        const uint64_t len = ((uint64_t)bytes[at] << 8) | bytes[at + 1];
        if (len > n - at - 2) break;
        if (frames < cap) {
            if (off_out) off_out[frames] = at + 2;
            if (size_out) size_out[frames] = len;
        }
        at += 2 + len; frames += 1;
    }
    if (used_out) *used_out = at;
    return frames;
}

#ifdef __HIPCC__
/* what k_rtpu_class found out about a packet */
struct alignas(16) RtpuRec {
    uint32_t bits;                  /* class | S << 3 | E << 4 | continues << 5 | marker << 6 | padding bytes << 8 | seq << 16 */
    uint32_t ts;
    uint32_t pay_off;               /* where the payload begins in the packet (below 2^19)                            */
    uint32_t chain;                 /* an FU: the number of its chain (k_rtpu_chain)                                  */
};

struct RtpuArgs {
    uint64_t n;                                       /* input bytes (the input is t.src)                            */
    const unsigned long long* pkt_off; const unsigned long long* pkt_size; uint64_t n_packets;
    RtpuRule q;
    uint64_t out_cap, nal_cap, au_cap;
    hbs_nal_entry* index_out; uint32_t* nal_au_out; unsigned long long* au_ts_out;      /* nullable                  */
    hbs_summary* summary;
    PieceTable t;                   /* a single NAL, a unit of an aggregation packet, a fragment: a piece each, with a literal
                                       (the start code; start code + the two rebuilt bytes on a chain's first packet; none on
                                       its other packets); t.tiles covers out_cap.  ctl: 0 error, 1 output bytes, 2 pieces,
                                       3 chains, 4 NALs, 5 breaks << 32 | dropped, 6 accepted packets                 */
    /* scratch (lay_rtpu) */
    RtpuRec* rec;                   /* n_packets                                                                      */
    unsigned long long* ap;         /* 2 per packet, written and read for aggregation packets only: units, NAL bytes  */
    uint32_t* chain_w;              /* 2 per chain (at most n_packets): its first packet has S, its last has E        */
    uint32_t* state;                /* n_packets: 1 an FU of a whole chain, 2 gives NALs (for a chain: its last packet), 4
                                       the chain's last packet, 8 its first NAL begins an access unit                 */
    unsigned long long* part_c;     /* 8 per block: chains begun, 1 + the lowest faulty packet                        */
    unsigned long long* part_n;     /* 8 per block: output bytes, NALs, pieces, breaks << 32 | dropped, accepted, 0   */
    unsigned long long* part_a;     /* 8 per block: access units begun, 0                                             */
    unsigned long long* last_n;     /* 1 per block: 1 + the last packet that gives NALs, then of the blocks in front  */
    hipEvent_t ev_begin, ev_end;
};

inline uint64_t rtpu_blocks(uint64_t n_packets) { return (n_packets + kRtpuPacketsPerBlock - 1) / kRtpuPacketsPerBlock; }

/* the scratch the call needs, sized by a.n_packets, a.nal_cap, a.out_cap (a.t.tiles) and whether there is an output */
inline void lay_rtpu(Carver& w, RtpuArgs& a)
{
    const uint64_t blocks = rtpu_blocks(a.n_packets);
    a.rec = w.take<RtpuRec>(a.n_packets * sizeof(RtpuRec));
    a.ap = w.take<unsigned long long>(a.n_packets * 16);
    a.chain_w = w.take<uint32_t>(a.n_packets * 8);
    a.state = w.take<uint32_t>(a.n_packets * 4);
    a.part_c = w.take<unsigned long long>(blocks * 64);
    a.part_n = w.take<unsigned long long>(blocks * 64);
    a.part_a = w.take<unsigned long long>(blocks * 64);
    a.last_n = w.take<unsigned long long>(blocks * 8);
    /* pieces: one a packet but for aggregation packets, whose pieces are NALs; a NAL takes startcode_bytes + 2 output bytes at
     * least, so more than out_cap / (startcode_bytes + 2) do not fit out_cap either (HBS_E_CAPACITY, nothing placed) */
    const uint64_t fit = a.out_cap / (a.q.sc + 2u);
    const uint64_t piece_cap = a.t.out ? a.n_packets + (a.nal_cap < fit ? a.nal_cap : fit) : 0;
    lay_pieces(w, a.t, piece_cap);
    a.t.piece_lit = w.take<unsigned long long>((piece_cap + 1) * 8);
}
hipError_t launch_rtp_unpack(const RtpuArgs& a, hipStream_t st);
#endif

} // namespace hbs
#endif
