/*
 * hbs_tsmux.h -- hbs_ts_mux (include/hevcbitstream_amd.h): the rule that turns one access unit into transport packets, as
 * ONE host/device inline function -- tsm_packet lays packet j of an AU out (header, adaptation field, PES header, source
 * range) and tsm_head_byte gives every byte in front of its ES bytes; the kernels of hbs_tsmux.hip, the two host entry
 * points and the tests all run them -- the PAT / PMT builder with its CRC, and the host-visible launcher.  Everything above
 * the launcher compiles with plain g++.
 */
#ifndef HBS_TSMUX_H
#define HBS_TSMUX_H

#include "hbs_ts.h"

namespace hbs {

constexpr int kTsmPlanLanes = 64;                   /* plan: one wavefront a workgroup ...                          */
constexpr int kTsmPlanPer = 4;                      /* ... a lane per four consecutive AUs                          */
constexpr int kTsmAusPerBlock = kTsmPlanLanes * kTsmPlanPer;
constexpr int kTsmPacketsPerBlock = 2048;           /* copy: output packets of one workgroup ...                    */
constexpr int kTsmRoundPackets = 256;               /* ... laid out 256 at a time, one a lane                       */
constexpr uint64_t kTsmNoTime = ~0ull;
constexpr uint64_t kTsmTimeMask = (1ull << 33) - 1;

/* what the rule needs to know of an AU */
struct TsmAu {
    uint64_t es_bytes;                               /* E                                                            */
    uint64_t pts, dts;                               /* as given (dts: ~0 without d_dts)                             */
    uint32_t f;                                      /* PTS_DTS_flags: 0, 2, 3                                       */
    bool pcr, irap;
};

HBS_HD bool tsm_times_ok(uint64_t pts, uint64_t dts)
{
    if (pts != kTsmNoTime && pts > kTsmTimeMask) return false;
    if (dts != kTsmNoTime && (dts > kTsmTimeMask || pts == kTsmNoTime)) return false;
    return true;
}
HBS_HD uint32_t tsm_time_fields(uint64_t pts, uint64_t dts)
{
    return (dts != kTsmNoTime && dts != pts) ? 3u : pts != kTsmNoTime ? 2u : 0u;
}
HBS_HD TsmAu tsm_au(uint64_t es_bytes, uint64_t pts, uint64_t dts, bool irap, uint32_t mux_flags)
{
    TsmAu u;
    u.es_bytes = es_bytes; u.pts = pts; u.dts = dts; u.f = tsm_time_fields(pts, dts);
    u.pcr = (mux_flags & HBS_TSMUX_PCR) != 0 && u.f != 0; u.irap = irap;
    return u;
}
HBS_HD uint32_t tsm_pes_header_bytes(uint32_t f) { return f == 3u ? 19u : f == 2u ? 14u : 9u; }     /* H  */
HBS_HD uint32_t tsm_first_af_bytes(bool pcr) { return pcr ? 8u : 2u; }                              /* A1 */

/* N(a) */
HBS_HD uint64_t tsm_au_packets(const TsmAu& u)
{
    const uint64_t T = tsm_pes_header_bytes(u.f) + u.es_bytes, R1 = 184u - tsm_first_af_bytes(u.pcr);
    return T <= R1 ? 1u : 1u + (T - R1 + 183u) / 184u;
}

/* is a PAT + PMT pair placed in front of AU a? */
HBS_HD bool tsm_psi_before(uint64_t a, bool irap, uint32_t mux_flags)
{
    if (mux_flags & HBS_TSMUX_NO_PSI) return false;
    return a == 0 || ((mux_flags & HBS_TSMUX_PSI_AT_IRAP) != 0 && irap);
}

/* packet j of an AU, 0 <= j < N(a) */
struct TsmPacket {
    uint32_t pusi;
    uint32_t afc;                /* 3: with an adaptation field, 1: without                                             */
    uint32_t afl;                /* adaptation_field_length (afc 3)                                                     */
    uint32_t af_flags;           /* its flags byte (afl >= 1)                                                           */
    uint32_t pes_bytes;          /* H in the first packet, else 0                                                       */
    uint32_t head;               /* transport bytes in front of the ES bytes: 4 + adaptation field + PES header         */
    uint64_t src_off;            /* the packet's ES bytes are [src_off, src_off + 188 - head) of the AU's               */
};

HBS_HD void tsm_packet(const TsmAu& u, uint64_t j, TsmPacket& r)
{
    const uint32_t H = tsm_pes_header_bytes(u.f), A1 = tsm_first_af_bytes(u.pcr), R1 = 184u - A1;
    const uint64_t T = H + u.es_bytes;
    if (j == 0) {
        r.pusi = 1; r.afc = 3;
        r.afl = T <= R1 ? 183u - (uint32_t)T : A1 - 1u;
        r.af_flags = (u.irap ? 0x40u : 0u) | (u.pcr ? 0x10u : 0u);
        r.pes_bytes = H;
        r.head = 5u + r.afl + H;
        r.src_off = 0;
        return;
    }
    r.pusi = 0; r.af_flags = 0; r.pes_bytes = 0;
    r.src_off = (uint64_t)(R1 - H) + (j - 1u) * 184u;
    const uint64_t left = u.es_bytes - r.src_off;                    /* >= 1 for j < N(a) */
    if (left >= 184u) { r.afc = 1; r.afl = 0; r.head = 4; }
    else { r.afc = 3; r.afl = 183u - (uint32_t)left; r.head = 5u + r.afl; }
}

/* byte k (0..4) of the five a PES time takes */
HBS_HD uint32_t tsm_stamp_byte(uint64_t t, uint32_t marker, uint32_t k)
{
    const uint32_t v = k == 0 ? ((marker << 4) | ((uint32_t)((t >> 30) & 7u) << 1) | 1u)
                     : k == 1 ? (uint32_t)(t >> 22)
                     : k == 2 ? (((uint32_t)((t >> 15) & 0x7Fu) << 1) | 1u)
                     : k == 3 ? (uint32_t)(t >> 7)
                     :          (((uint32_t)(t & 0x7Fu) << 1) | 1u);
    return v & 0xFFu;
}

/* transport byte i of the packet, i < p.head: the header, the adaptation field, the PES header */
HBS_HD uint32_t tsm_head_byte(const TsmAu& u, const TsmPacket& p, uint32_t pid, uint64_t pcr_lead, uint32_t cc, uint32_t i)
{
    if (i < 4u)
        return i == 0 ? 0x47u : i == 1 ? ((p.pusi << 6) | (pid >> 8)) : i == 2 ? (pid & 0xFFu) : ((p.afc << 4) | (cc & 15u));
    i -= 4u;
    if (p.afc & 2u) {
        if (i == 0) return p.afl;
        if (i <= p.afl) {
            if (i == 1u) return p.af_flags;
            if ((p.af_flags & 0x10u) && i < 8u) {
                const uint64_t base = ((u.f == 3u ? u.dts : u.pts) - pcr_lead) & kTsmTimeMask;
                const uint32_t k = i - 2u;
                const uint32_t v = k == 0 ? (uint32_t)(base >> 25) : k == 1 ? (uint32_t)(base >> 17) : k == 2 ? (uint32_t)(base >> 9)
                                 : k == 3 ? (uint32_t)(base >> 1) : k == 4 ? (((uint32_t)(base & 1u) << 7) | 0x7Eu) : 0u;
                return v & 0xFFu;
            }
            return 0xFFu;
        }
        i -= 1u + p.afl;
    }
    if (i < 9u) {
        if (i == 7u) return u.f << 6;
        if (i == 8u) return p.pes_bytes - 9u;
        return (uint32_t)((0x00840000E0010000ull >> (8u * i)) & 0xFFu);               /* 00 00 01 E0 00 00 84, byte 0 lowest */
    }
    if (i < 14u) return tsm_stamp_byte(u.pts, u.f == 3u ? 3u : 2u, i - 9u);
    return tsm_stamp_byte(u.dts, 1u, i - 14u);
}

/* ---- host side: parameters, PAT / PMT, one packet ---------------------------------------------------------------------- */

inline bool tsm_params_ok(const hbs_ts_mux_params* p)
{
    if (!p || !ts_packet_bytes_ok(p->packet_bytes)) return false;
    if (p->pid < 16 || p->pid > 8190 || p->pmt_pid < 16 || p->pmt_pid > 8190 || p->pid == p->pmt_pid) return false;
    if (p->program_number < 1 || p->program_number > 65535 || p->transport_stream_id < 0 || p->transport_stream_id > 65535) return false;
    if (p->flags & ~(HBS_TSMUX_PCR | HBS_TSMUX_PSI_AT_IRAP | HBS_TSMUX_NO_PSI)) return false;
    return p->cc_es <= 15u && p->cc_pat <= 15u && p->cc_pmt <= 15u && p->reserved == 0u;
}

/* MPEG-2 CRC-32: polynomial 0x04C11DB7, initial value 0xFFFFFFFF, not reflected, no final xor */
inline uint32_t tsm_crc32(const uint8_t* b, uint32_t n)
{
    uint32_t crc = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < n; ++i) {
        crc ^= (uint32_t)b[i] << 24;
        for (int k = 0; k < 8; ++k) crc = (crc & 0x80000000u) ? (crc << 1) ^ 0x04C11DB7u : crc << 1;
    }
    return crc;
}

/* a section packet: header with payload_unit_start, pointer_field 0, the section with its CRC, FF to the end */
inline void tsm_section_packet(uint8_t out[188], uint32_t pid, uint32_t cc, const uint8_t* body, uint32_t n)
{
    out[0] = 0x47; out[1] = (uint8_t)(0x40u | (pid >> 8)); out[2] = (uint8_t)(pid & 0xFFu); out[3] = (uint8_t)(0x10u | (cc & 15u));
    out[4] = 0;
    for (uint32_t i = 0; i < n; ++i) out[5 + i] = body[i];
    const uint32_t crc = tsm_crc32(body, n);
    out[5 + n] = (uint8_t)(crc >> 24); out[6 + n] = (uint8_t)(crc >> 16); out[7 + n] = (uint8_t)(crc >> 8); out[8 + n] = (uint8_t)crc;
    for (uint32_t i = 9 + n; i < kTsBytes; ++i) out[i] = 0xFF;
}

inline int tsm_psi_host(const hbs_ts_mux_params* p, uint8_t pat[188], uint8_t pmt[188])
{
    if (!pat || !pmt || !tsm_params_ok(p)) return HBS_E_ARG;
    const uint32_t pid = (uint32_t)p->pid, pmt_pid = (uint32_t)p->pmt_pid, prog = (uint32_t)p->program_number, tsid = (uint32_t)p->transport_stream_id;
    const uint8_t a[12] = {0x00, 0xB0, 0x0D, (uint8_t)(tsid >> 8), (uint8_t)tsid, 0xC1, 0x00, 0x00, (uint8_t)(prog >> 8), (uint8_t)prog,
                           (uint8_t)(0xE0u | (pmt_pid >> 8)), (uint8_t)pmt_pid};
    const uint8_t m[23] = {0x02, 0xB0, 0x18, (uint8_t)(prog >> 8), (uint8_t)prog, 0xC1, 0x00, 0x00, (uint8_t)(0xE0u | (pid >> 8)), (uint8_t)pid,
                           0xF0, 0x00, 0x24, (uint8_t)(0xE0u | (pid >> 8)), (uint8_t)pid, 0xF0, 0x06, 0x05, 0x04, 'H', 'E', 'V', 'C'};
    tsm_section_packet(pat, 0u, p->cc_pat, a, 12);
    tsm_section_packet(pmt, pmt_pid, p->cc_pmt, m, 23);
    return 0;
}

inline uint64_t tsm_au_packets_host(uint64_t es_bytes, int time_fields, int pcr)
{
    if (time_fields < 0 || time_fields > 2) return 0;
    TsmAu u;
    u.es_bytes = es_bytes; u.pts = u.dts = 0; u.f = time_fields == 0 ? 0u : (uint32_t)time_fields + 1u;
    u.pcr = pcr != 0 && u.f != 0; u.irap = false;
    return tsm_au_packets(u);
}

/* the 188 transport bytes of packet j of an AU whose ES bytes are es[0, u.es_bytes): the rule run byte by byte */
inline void tsm_write_packet_host(const TsmAu& u, const uint8_t* es, uint64_t j, uint32_t pid, uint64_t pcr_lead, uint32_t cc, uint8_t out[188])
{
    TsmPacket p;
    tsm_packet(u, j, p);
    for (uint32_t i = 0; i < p.head; ++i) out[i] = (uint8_t)tsm_head_byte(u, p, pid, pcr_lead, cc, i);
    for (uint32_t i = p.head; i < kTsBytes; ++i) out[i] = es[p.src_off + (i - p.head)];
}

#ifdef __HIPCC__
struct TsmPsi { uint32_t w[2][kTsBytes / 4]; };      /* the PAT and the PMT packet of pair 0, as little-endian words */

struct TsmArgs {
    const uint8_t* src; uint64_t n;                   /* the Annex-B stream                                           */
    const hbs_access_unit* au; uint64_t n_aus;
    const unsigned long long* pts; const unsigned long long* dts;     /* nullable                                     */
    uint32_t B, lead, pid, flags, cc_es, cc_pat, cc_pmt;
    uint64_t pcr_lead;
    uint8_t* out; uint64_t out_cap;                   /* out NULL: plan only                                          */
    uint32_t* au_packet;                              /* nullable                                                     */
    hbs_summary* summary;
    /* scratch (lay_tsm) */
    unsigned long long* part;      /* 8 per plan block: ES packets, PSI pairs, ES bytes, 1 + the lowest bad AU (0: none)          */
    unsigned long long* ctl;       /* 8: error, packets                                                                            */
    uint32_t* au_pkt;              /* n_aus + 1: the packet AU a's PES begins in (then the total)                                  */
    uint32_t* es_pkt;              /* n_aus + 1: ES packets in front of AU a (then the total)                                      */
    uint32_t* blk_first;           /* copy_blocks: the last AU whose PES begins at or in front of the block's first packet (0: none) */
    uint64_t copy_blocks;          /* workgroups of the copy: what out_cap and the stream can hold                                 */
    TsmPsi psi;
    hipEvent_t ev_begin, ev_end;
};

/* the most packets a call can make: N(a) <= 2 + E / 184, a pair in front of every AU, the AUs' bytes disjoint */
inline uint64_t tsm_packet_bound(uint64_t n_aus, uint64_t stream_bytes)
{
    const uint64_t b = 4u * n_aus + stream_bytes / 184u + 1u;
    return b < 0xFFFFFFFFull ? b : 0xFFFFFFFFull;
}

inline void lay_tsm(Carver& w, TsmArgs& a)
{
    const uint64_t blocks = (a.n_aus + kTsmAusPerBlock - 1) / kTsmAusPerBlock;
    a.part = w.take<unsigned long long>(blocks * 64);
    a.ctl = w.take<unsigned long long>(64);
    const uint64_t tabs = a.out ? a.n_aus + 1 : 0;                  /* (a plan-only call places nothing) */
    a.au_pkt = w.take<uint32_t>(tabs * 4);
    a.es_pkt = w.take<uint32_t>(tabs * 4);
    a.blk_first = w.take<uint32_t>(a.copy_blocks * 4);
}
hipError_t launch_ts_mux(const TsmArgs& a, hipStream_t st);
#endif

} // namespace hbs
#endif
