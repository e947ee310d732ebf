/*
 * hbs_rtp.h -- hbs_rtp_pack (include/hevcbitstream_amd.h): the rule that turns one NAL unit into RFC 7798 RTP packets, as
 * host/device inline functions -- rtp_nal lays a NAL out (single NAL unit packet or fragmentation units, packets, output
 * bytes), rtp_packet_bytes gives packet p's length and rtp_head_byte every byte in front of its NAL bytes; with
 * HBS_RTP_AGGREGATE rtp_group_next is the greedy group rule and rtp_ap_head_byte every byte in front of an aggregation
 * packet's first unit; the kernels of
 * hbs_rtp.hip, the two host entry points and the tests all run them -- the receiver's view of one packet (rtp_packet_rule: a
 * host/device function too, behind rtp_packet_host and in the kernels of hbs_rtp_unpack, hbs_rtpun.hip), and the host-visible
 * launcher.  Everything above the launcher compiles with plain g++.
 */
#ifndef HBS_RTP_H
#define HBS_RTP_H

#include "hbs_common.h"

namespace hbs {

constexpr int kRtpPlanLanes = 256;                  /* plan: a lane a NAL, 256 NALs a workgroup                     */
constexpr int kRtpNalsPerBlock = kRtpPlanLanes;
constexpr uint64_t kRtpTileBytes = 64 * 1024;       /* copy: output bytes of one workgroup                          */
constexpr uint32_t kRtpHeader = 12;                 /* the fixed RTP header                                         */
constexpr uint32_t kRtpFuHeader = 3;                /* PayloadHdr (2) + FU header (1)                               */
constexpr int kRtpMinPayload = 4, kRtpMaxPayload = 65535 - 12;
constexpr uint64_t kRtpTimeLimit = 1ull << 33;      /* a d_pts value must be below this                             */

/* what of hbs_rtp_params the rule reads */
struct RtpRule {
    uint32_t mp;                                     /* max_payload                                                  */
    uint32_t fr;                                     /* framing: 0 or 2                                              */
    uint32_t pt, ssrc, seq;
};

HBS_HD bool rtp_max_payload_ok(int64_t mp) { return mp >= kRtpMinPayload && mp <= kRtpMaxPayload; }

/* NAL of L >= 2 bytes */
struct RtpNal {
    bool fu;                                         /* L > mp                                                       */
    uint64_t packets;                                /* 1, or n = ceil((L - 2) / (mp - 3)) >= 2                      */
    uint64_t out_bytes;                              /* framing, headers and NAL bytes of all its packets            */
};

HBS_HD RtpNal rtp_nal(uint64_t L, uint32_t mp, uint32_t fr)
{
    RtpNal r;
    r.fu = L > mp;
    if (!r.fu) { r.packets = 1; r.out_bytes = fr + kRtpHeader + L; return r; }
    const uint64_t F = mp - 3u, B = L - 2u;
    r.packets = (B + F - 1u) / F;
    r.out_bytes = r.packets * (uint64_t)(fr + kRtpHeader + kRtpFuHeader) + B;
    return r;
}

/* every packet of an FU NAL but its last takes this many output bytes */
HBS_HD uint32_t rtp_full_packet_bytes(const RtpRule& q) { return q.fr + kRtpHeader + q.mp; }

/* output bytes of packet p of the NAL (p < packets), the length field included */
HBS_HD uint64_t rtp_packet_bytes(const RtpRule& q, uint64_t L, const RtpNal& u, uint64_t p)
{
    if (!u.fu) return u.out_bytes;
    if (p + 1 < u.packets) return rtp_full_packet_bytes(q);
    return (uint64_t)(q.fr + kRtpHeader + kRtpFuHeader) + (L - 2u) - p * (uint64_t)(q.mp - 3u);
}

/* bytes in front of the NAL bytes a packet carries */
HBS_HD uint32_t rtp_head_bytes(const RtpRule& q, bool fu) { return q.fr + kRtpHeader + (fu ? kRtpFuHeader : 0u); }

/* where in the NAL the bytes of packet p begin */
HBS_HD uint64_t rtp_packet_src(const RtpRule& q, bool fu, uint64_t p) { return fu ? 2u + p * (uint64_t)(q.mp - 3u) : 0u; }

/* byte i (i < rtp_head_bytes) of a packet of plen bytes (length field included): number j of the call, timestamp ts;
 * last: the NAL's last packet; marker: the NAL ends its access unit; h0, h1: the NAL's header (read for an FU only) */
HBS_HD uint32_t rtp_head_byte(const RtpRule& q, bool fu, bool first, bool last, bool marker, uint64_t plen, uint64_t j, uint32_t ts,
                              uint32_t h0, uint32_t h1, uint32_t i)
{
    if (i < q.fr) {
        const uint32_t len = (uint32_t)(plen - q.fr);
        return (i == 0 ? len >> 8 : len) & 0xFFu;
    }
    i -= q.fr;
    if (i < kRtpHeader) {
        const uint32_t s = (q.seq + (uint32_t)j) & 0xFFFFu;
        switch (i) {
        case 0: return 0x80u;
        case 1: return ((last && marker) ? 0x80u : 0u) | q.pt;
        case 2: return s >> 8;
        case 3: return s & 0xFFu;
        case 4: case 5: case 6: case 7: return (ts >> (8u * (7u - i))) & 0xFFu;
        default: return (q.ssrc >> (8u * (11u - i))) & 0xFFu;
        }
    }
    i -= kRtpHeader;                                                 /* an FU's three bytes */
    if (i == 0) return (h0 & 0x81u) | 0x62u;
    if (i == 1) return h1;
    return (first ? 0x80u : 0u) | (last ? 0x40u : 0u) | ((h0 >> 1) & 63u);
}

/* ---- aggregation packets (HBS_RTP_AGGREGATE): the group rule and the bytes in front of an AP's first unit -------------- */

constexpr uint32_t kRtpApHead = 2;                  /* an AP's PayloadHdr                                           */
constexpr uint32_t kRtpApSize = 2;                  /* the size field in front of every unit                        */
static_assert(HBS_RTP_AP_SPAN == kRtpNalsPerBlock, "a plan workgroup finds its groups without looking outside its NALs");

/* what NAL k adds to an AP's payload, 2 + L; a NAL too long for any packet counts as 65538 so that 256 of them sum in 32 bits */
HBS_HD uint32_t rtp_ap_weight(uint64_t L) { return kRtpApSize + (uint32_t)(L < 0x10000u ? L : 0x10000u); }

/* a NAL of weight w that shares a packet with no other NAL whatever its neighbours are: 2 + w + (2 + 2) > mp */
HBS_HD bool rtp_ap_loner(uint32_t w, uint32_t mp) { return (uint64_t)kRtpApHead + w + kRtpApSize + 2u > mp; }

/* next(i) of the group rule for i < hi: the smallest j > i with j == hi, au(j) != au(i) or 2 + sum_{m = i..j} (2 + L_m) > mp.
 * hi: the end of i's span of HBS_RTP_AP_SPAN NALs or n_nals, whichever is lower; pre(j): the sum of rtp_ap_weight over the
 * NALs in front of j, from any fixed NAL at or in front of i (pre(hi) exists); au(j): NAL j's AU number.  AU numbers never go
 * down and weights are positive, so "j ends the group" holds for every j behind the first for which it holds: a binary search.
 * (Where the AU numbers do go down, which the call refuses, the result is still in (i, hi].) */
template <class Pre, class Au> HBS_HD uint32_t rtp_group_next(uint32_t i, uint32_t hi, uint32_t mp, Pre pre, Au au)
{
    const uint64_t base = pre(i);
    const uint32_t a = au(i);
    uint32_t lo = i + 1, top = hi;                                   /* the answer lies in [lo, top] */
    while (lo < top) {
        const uint32_t mid = lo + ((top - lo) >> 1);
        const bool ends = au(mid) != a || (uint64_t)kRtpApHead + (pre(mid + 1) - base) > mp;
        if (ends) top = mid; else lo = mid + 1;
    }
    return lo;
}

/* F, layer id and TID of an AP's PayloadHdr: the OR of the units' F bits, the lowest layer id, the lowest TID.  `acc` starts
 * as kRtpApFoldStart and takes every unit's header bytes; then rtp_ap_payload_hdr */
constexpr uint32_t kRtpApFoldStart = 63u << 8 | 7u;                  /* F << 16 | layer << 8 | tid */
HBS_HD uint32_t rtp_ap_fold(uint32_t acc, uint32_t h0, uint32_t h1)
{
    const uint32_t f = (acc >> 16) | (h0 >> 7), layer = (h0 & 1u) << 5 | h1 >> 3, tid = h1 & 7u;
    const uint32_t l0 = (acc >> 8) & 63u, t0 = acc & 7u;
    return f << 16 | (layer < l0 ? layer : l0) << 8 | (tid < t0 ? tid : t0);
}
/* -> byte 0 | byte 1 << 8 */
HBS_HD uint32_t rtp_ap_payload_hdr(uint32_t acc)
{
    const uint32_t f = acc >> 16, layer = (acc >> 8) & 63u, tid = acc & 7u;
    return (f << 7 | 48u << 1 | layer >> 5) | ((layer & 31u) << 3 | tid) << 8;
}

/* bytes in front of the NAL bytes of an AP's first unit, and of a later unit */
HBS_HD uint32_t rtp_ap_first_head(const RtpRule& q) { return q.fr + kRtpHeader + kRtpApHead + kRtpApSize; }

/* byte i (i < rtp_ap_first_head) of an AP whose payload has pay bytes: number j of the call, timestamp ts; marker: its last
 * unit ends its access unit; hdr: rtp_ap_payload_hdr; L: the first unit's size */
HBS_HD uint32_t rtp_ap_head_byte(const RtpRule& q, bool marker, uint32_t pay, uint64_t j, uint32_t ts, uint32_t hdr, uint32_t L, uint32_t i)
{
    const uint32_t fixed = q.fr + kRtpHeader;
    if (i < fixed) return rtp_head_byte(q, false, true, true, marker, (uint64_t)fixed + pay, j, ts, 0, 0, i);
    i -= fixed;
    if (i < kRtpApHead) return (hdr >> (8u * i)) & 0xFFu;
    return (i == kRtpApHead ? L >> 8 : L) & 0xFFu;
}

/* ---- host side: parameters, one NAL, one packet as a receiver reads it ------------------------------------------------- */

inline bool rtp_params_ok(const hbs_rtp_params* p)
{
    if (!p || !rtp_max_payload_ok(p->max_payload)) return false;
    if (p->payload_type < 0 || p->payload_type > 127 || (p->framing != 0 && p->framing != 2)) return false;
    return (p->flags & ~(HBS_RTP_OPEN_END | HBS_RTP_AGGREGATE)) == 0u && p->seq <= 0xFFFFu;
}

inline RtpRule rtp_rule(const hbs_rtp_params* p)
{
    RtpRule q;
    q.mp = (uint32_t)p->max_payload; q.fr = (uint32_t)p->framing; q.pt = (uint32_t)p->payload_type; q.ssrc = p->ssrc; q.seq = p->seq;
    return q;
}

inline uint64_t rtp_nal_packets_host(uint64_t nal_bytes, int max_payload)
{
    if (nal_bytes < 2 || !rtp_max_payload_ok(max_payload)) return 0;
    return rtp_nal(nal_bytes, (uint32_t)max_payload, 0).packets;
}

/* packet p of the NAL nal[0, L) into out[0, rtp_packet_bytes): the rule run byte by byte */
inline void rtp_write_packet_host(const RtpRule& q, const uint8_t* nal, uint64_t L, uint64_t p, bool marker, uint64_t j, uint32_t ts, uint8_t* out)
{
    const RtpNal u = rtp_nal(L, q.mp, q.fr);
    const uint64_t plen = rtp_packet_bytes(q, L, u, p);
    const uint32_t head = rtp_head_bytes(q, u.fu);
    const uint64_t src = rtp_packet_src(q, u.fu, p);
    for (uint32_t i = 0; i < head; ++i)
        out[i] = (uint8_t)rtp_head_byte(q, u.fu, p == 0, p + 1 == u.packets, marker, plen, j, ts, nal[0], nal[1], i);
    for (uint64_t i = head; i < plen; ++i) out[i] = nal[src + (i - head)];
}

/* one RTP packet of n bytes (no length field) as a receiver reads it: RFC 3550 5.1 / 5.3.1, RFC 7798 4.4.  byte(i) is byte i of
 * the packet; none at or beyond n is asked for.  The one rule of hbs_rtp_packet_host and of the kernels of hbs_rtp_unpack
 * (hbs_rtpun.hip), which keep a packet's first bytes in registers */
template <class B> HBS_HD int rtp_packet_rule(B byte, uint64_t n, hbs_rtp_packet* out)
{
    if (n < kRtpHeader) return HBS_E_ARG;
    const uint32_t b0 = byte(0), b1 = byte(1);
    if ((b0 >> 6) != 2u) return HBS_E_ARG;
    uint64_t head = kRtpHeader + 4u * (b0 & 15u);                    /* the CSRC entries */
    if (head > n) return HBS_E_ARG;
    if (b0 & 0x10u) {                                                /* a header extension: 16 bits of profile, 16 of length in words */
        if (n - head < 4u) return HBS_E_ARG;
        const uint64_t words = ((uint64_t)byte(head + 2) << 8) | byte(head + 3);
        head += 4u;
        if (n - head < 4u * words) return HBS_E_ARG;
        head += 4u * words;
    }
    uint64_t pad = 0;
    if (b0 & 0x20u) {                                                /* padding: its last byte counts it, itself included */
        pad = byte(n - 1);
        if (pad == 0 || pad > n - head) return HBS_E_ARG;
    }
    hbs_rtp_packet r;
    r.payload_off = head; r.payload_len = n - head - pad;
    r.marker = b1 >> 7; r.payload_type = b1 & 127u;
    r.seq = (byte(2) << 8) | byte(3);
    r.timestamp = (byte(4) << 24) | (byte(5) << 16) | (byte(6) << 8) | byte(7);
    r.ssrc = (byte(8) << 24) | (byte(9) << 16) | (byte(10) << 8) | byte(11);
    r.kind = HBS_RTP_OTHER; r.nal_type = -1; r.fu_start = r.fu_end = 0;
    r.nal_off = r.payload_off; r.nal_len = r.payload_len;
    r.nal_header[0] = r.nal_header[1] = 0; r.reserved[0] = r.reserved[1] = 0;
    if (r.payload_len >= 2) {
        const uint32_t p0 = byte(head), p1 = byte(head + 1);
        const uint32_t t = (p0 >> 1) & 63u;
        r.nal_type = (int32_t)t; r.nal_header[0] = (uint8_t)p0; r.nal_header[1] = (uint8_t)p1;
        if (t < 48u) {
            r.kind = HBS_RTP_SINGLE;
        } else if (t == 48u) {
            r.kind = HBS_RTP_AP;
        } else if (t == 49u) {
            if (r.payload_len < kRtpFuHeader) return HBS_E_ARG;
            const uint32_t p2 = byte(head + 2);
            r.kind = HBS_RTP_FU;
            r.fu_start = p2 >> 7; r.fu_end = (p2 >> 6) & 1u;
            r.nal_type = (int32_t)(p2 & 63u);
            r.nal_header[0] = (uint8_t)((p0 & 0x81u) | ((p2 & 63u) << 1));
            r.nal_off = head + kRtpFuHeader; r.nal_len = r.payload_len - kRtpFuHeader;
        }
    }
    *out = r;
    return 0;
}

/* bytes in memory: byte i of the packet at p */
struct RtpBytesAt {
    const uint8_t* p;
    HBS_M uint32_t operator()(uint64_t i) const { return p[i]; }
};

inline int rtp_packet_host(const uint8_t* pkt, uint64_t n, hbs_rtp_packet* out)
{
    if (!pkt || !out) return HBS_E_ARG;
    return rtp_packet_rule(RtpBytesAt{pkt}, n, out);
}

#ifdef __HIPCC__
} // namespace hbs
#include <hip/hip_runtime_api.h>
namespace hbs {

struct RtpArgs {
    const uint8_t* src; uint64_t n;                   /* the stream                                                   */
    const hbs_nal_entry* index; uint64_t n_nals;
    const uint32_t* nal_au; uint64_t n_aus;           /* nal_au NULL: one access unit                                 */
    const unsigned long long* pts;                    /* nullable                                                     */
    RtpRule q;
    uint32_t flags, ts_base, ts_step;
    uint8_t* out; uint64_t out_cap;                   /* out NULL: plan only                                          */
    unsigned long long* nal_off;                      /* nullable, n_nals + 1                                         */
    unsigned long long* nal_packet;                   /* nullable, n_nals + 1                                         */
    hbs_summary* summary;
    /* scratch (lay_rtp) */
    unsigned long long* part;      /* 8 per plan block: output bytes, packets, NAL bytes, FU NALs, 1 + the lowest bad NAL (0: none) */
    unsigned long long* ctl;       /* 8: error, output bytes, packets                                                               */
    unsigned long long* rec_out;   /* n_nals + 1: output offset of NAL k's first packet (then the total)                            */
    unsigned long long* rec_pkt;   /* n_nals + 1: number of NAL k's first packet (then the total)                                   */
    unsigned long long* rec_src;   /* n_nals: start_k                                                                                */
    unsigned long long* rec_len;   /* n_nals: L; with HBS_RTP_AGGREGATE bits 62..63: 0 a packet or FUs of its own, 1 an AP's first unit, 2 a later unit */
    unsigned long long* rec_tm;    /* n_nals: the timestamp, bit 32: the NAL ends its access unit (an AP's first unit: its last unit does) */
    uint32_t* rec_ap;              /* n_nals, with HBS_RTP_AGGREGATE only; an AP's first unit: payload bytes | rtp_ap_payload_hdr << 16 */
    unsigned long long* tile_first;/* tiles + 1: the NAL the output tile's first byte lies in                                       */
    uint64_t tiles;                /* output tiles the copy's grid covers                                                           */
    hipEvent_t ev_begin, ev_end;
};

/* the most output bytes a call can make: L + 15 + framing for a single packet, a head of 15 + framing for every mp - 3 bytes
 * of an FU and one more for its short last packet.  HBS_RTP_AGGREGATE never makes more: an AP of m units takes
 * (m - 1)(framing + 12) - 2 - 2m >= 6 bytes less than its m single packets, so the bound and the tile count hold for it too */
inline uint64_t rtp_output_bound(uint64_t n_nals, uint64_t stream_bytes, const RtpRule& q)
{
    const uint64_t head = q.fr + kRtpHeader + kRtpFuHeader;
    return stream_bytes + head * (2u * n_nals + stream_bytes / (q.mp - 3u));
}

inline uint64_t rtp_tiles(uint64_t reach)
{
    const uint64_t t = reach / kRtpTileBytes + (reach % kRtpTileBytes ? 1 : 0);
    return t < 0x7FFFFFFFull ? t : 0x7FFFFFFFull;
}

inline void lay_rtp(Carver& w, RtpArgs& a)
{
    const uint64_t blocks = (a.n_nals + kRtpNalsPerBlock - 1) / kRtpNalsPerBlock;
    a.part = w.take<unsigned long long>(blocks * 64);
    a.ctl = w.take<unsigned long long>(64);
    const uint64_t recs = a.out ? a.n_nals : 0;                      /* (a plan-only call places nothing) */
    a.rec_out = w.take<unsigned long long>(a.out ? (recs + 1) * 8 : 0);
    a.rec_pkt = w.take<unsigned long long>(a.out ? (recs + 1) * 8 : 0);
    a.rec_src = w.take<unsigned long long>(recs * 8);
    a.rec_len = w.take<unsigned long long>(recs * 8);
    a.rec_tm = w.take<unsigned long long>(recs * 8);
    a.rec_ap = w.take<uint32_t>((a.flags & HBS_RTP_AGGREGATE) ? recs * 4 : 0);
    a.tile_first = w.take<unsigned long long>(a.tiles ? (a.tiles + 1) * 8 : 0);
}
hipError_t launch_rtp_pack(const RtpArgs& a, hipStream_t st);
#endif

} // namespace hbs
#endif
