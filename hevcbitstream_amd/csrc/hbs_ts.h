/*
 * hbs_ts.h -- hbs_ts_demux (include/hevcbitstream_amd.h): the rule that turns the bytes of one MPEG transport packet
 * (ISO/IEC 13818-1) into a record, as ONE host/device inline function -- the kernels of hbs_ts.hip, hbs_ts_packet_host and
 * the tests all run ts_classify -- the PAT / PMT walk of hbs_ts_find_pid_host, and the host-visible launcher.  Everything
 * above the launcher compiles with plain g++.
 */
#ifndef HBS_TS_H
#define HBS_TS_H

#include "hbs_common.h"

namespace hbs {

constexpr int kTsPacketsPerBlock = 2048;            /* plan and copy: 256 lanes x 8 packets                        */
constexpr int kTsRoundPackets = 256;                /* copy: packets whose source span is staged in LDS at a time  */
constexpr uint32_t kTsBytes = 188;                  /* transport bytes of a packet                                  */

HBS_HD bool ts_packet_bytes_ok(int B) { return B == 188 || B == 192 || B == 204; }
/* where the 188 transport bytes begin inside a packet of B bytes (192: behind the M2TS time prefix) */
HBS_HD uint32_t ts_lead(int B) { return B == 192 ? 4u : 0u; }
HBS_HD bool ts_has_es(int32_t cls) { return cls == HBS_TS_PAYLOAD || cls == HBS_TS_PES_START; }

/* a 33-bit PES time stamp from its five bytes (marker bits are not checked) */
HBS_HD uint64_t ts_stamp(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3, uint32_t x4)
{
    return ((uint64_t)((x0 >> 1) & 7u) << 30) | ((uint64_t)x1 << 22) | ((uint64_t)(x2 >> 1) << 15) | ((uint64_t)x3 << 7) | (x4 >> 1);
}

/*
 * The packet rule.  b(i) = transport byte i of the packet (0 <= i < 188); only the bytes the packet's class needs are asked
 * for, each at most a few times.  A fault leaves everything but cls and pid at "nothing".
 */
template <class Bytes>
HBS_HD void ts_classify(Bytes b, int want_pid, hbs_ts_packet& r)
{
    r.cls = HBS_TS_FAULT; r.pid = 0;
    r.off = r.len = r.es_off = r.es_len = 0; r.cc = 0; r.flags = 0;
    r.pts = r.dts = ~0ull;
    if (b(0) != 0x47u) return;                                   /* sync fault, whatever the PID */
    const uint32_t b1 = b(1);
    r.pid = ((b1 & 0x1Fu) << 8) | b(2);
    if ((int)r.pid != want_pid) { r.cls = HBS_TS_OTHER; return; }
    const uint32_t b3 = b(3);
    if ((b1 >> 7) || (b3 >> 6)) { r.cls = HBS_TS_SKIPPED; return; }   /* transport_error_indicator, scrambled */
    const uint32_t afc = (b3 >> 4) & 3u;
    uint32_t off = 4, flags = 0;
    if (afc & 2u) {
        const uint32_t afl = b(4);
        if (afl > 183u) return;
        off = 5 + afl;
        if (afl >= 1u) {
            const uint32_t f = b(5);
            if (f & 0x80u) flags |= HBS_TS_DISCONTINUITY;
            if (f & 0x40u) flags |= HBS_TS_RANDOM_ACCESS;
        }
    }
    if (!(afc & 1u) || off == kTsBytes) {
        r.cls = HBS_TS_NO_PAYLOAD; r.cc = b3 & 15u; r.off = off; r.flags = flags;
        return;
    }
    const uint32_t len = kTsBytes - off;
    uint32_t es_off = off, es_len = len;
    uint64_t pts = ~0ull, dts = ~0ull;
    const bool pusi = ((b1 >> 6) & 1u) != 0;
    if (pusi) {                                                  /* the payload begins a PES packet: q[i] = b(off + i) */
        if (len < 9u) return;
        if (b(off) != 0u || b(off + 1) != 0u || b(off + 2) != 1u) return;
        const uint32_t q6 = b(off + 6), f = b(off + 7) >> 6, q8 = b(off + 8);
        const uint32_t H = 9 + q8;
        if ((q6 & 0xC0u) != 0x80u || f == 1u || H > len) return;
        if ((f == 2u && q8 < 5u) || (f == 3u && q8 < 10u)) return;
        if (f >= 2u) {
            pts = dts = ts_stamp(b(off + 9), b(off + 10), b(off + 11), b(off + 12), b(off + 13));
            flags |= HBS_TS_PTS;
        }
        if (f == 3u) {
            dts = ts_stamp(b(off + 14), b(off + 15), b(off + 16), b(off + 17), b(off + 18));
            flags |= HBS_TS_DTS;
        }
        if (q6 & 4u) flags |= HBS_TS_DATA_ALIGNED;
        es_off = off + H; es_len = len - H;
    }
    r.cls = pusi ? HBS_TS_PES_START : HBS_TS_PAYLOAD;
    r.off = off; r.len = len; r.es_off = es_off; r.es_len = es_len; r.cc = b3 & 15u; r.flags = flags;
    r.pts = pts; r.dts = dts;
}

struct TsByteReader {
    const uint8_t* p;
    HBS_M uint32_t operator()(uint32_t i) const { return p[i]; }
};

/* ---- host side: one packet, and the PAT / PMT walk ------------------------------------------------------------------ */

inline int ts_packet_host(const uint8_t* packet, int packet_bytes, int pid, hbs_ts_packet* out)
{
    if (!packet || !out || !ts_packet_bytes_ok(packet_bytes) || pid < 0 || pid > 8191) return HBS_E_ARG;
    ts_classify(TsByteReader{packet + ts_lead(packet_bytes)}, pid, *out);
    return 0;
}

/* the section a packet of `pid` with payload_unit_start begins, when it has `table_id`: s = transport byte of the table_id,
 * e = one past the section's last byte (its CRC included).  0: not such a packet; -1: the section does not lie inside the
 * packet; 1: found.  Every length is bounded against the 188 bytes before it is used. */
inline int ts_section_in_packet(const uint8_t* b, int pid, uint32_t table_id, uint32_t min_body, uint32_t* s_out, uint32_t* e_out)
{
    /* (a section packet is no PES packet: ts_classify would report its payload_unit_start as a PES fault) */
    if (b[0] != 0x47u || (int)(((b[1] & 0x1Fu) << 8) | b[2]) != pid) return 0;
    if ((b[1] >> 7) || (b[3] >> 6) || !((b[1] >> 6) & 1u)) return 0;
    const uint32_t afc = (b[3] >> 4) & 3u;
    uint32_t off = 4;
    if (afc & 2u) { if (b[4] > 183u) return 0; off = 5u + b[4]; }
    if (!(afc & 1u) || off >= kTsBytes) return 0;
    const uint32_t s = off + 1u + b[off];                        /* behind the pointer_field */
    if (s >= kTsBytes) return -1;
    if (b[s] != table_id) return 0;
    if (s + 3u > kTsBytes) return -1;
    const uint32_t e = s + 3u + (((b[s + 1] & 0x0Fu) << 8) | b[s + 2]);
    if (e > kTsBytes || e < s + min_body + 4u) return -1;
    *s_out = s; *e_out = e;
    return 1;
}

inline int ts_find_pid_host(const uint8_t* bytes, uint64_t n, int packet_bytes, int stream_type, int* program_out)
{
    if (!ts_packet_bytes_ok(packet_bytes) || (n && !bytes)) return -1;
    const uint64_t B = (uint64_t)packet_bytes, packets = n / B;
    const uint32_t h = ts_lead(packet_bytes);
    int pmt_pid = -1, program = 0;
    for (uint64_t p = 0; p < packets && pmt_pid < 0; ++p) {      /* the first PAT section */
        const uint8_t* b = bytes + p * B + h;
        uint32_t s, e;
        const int rc = ts_section_in_packet(b, 0, 0u, 8u, &s, &e);
        if (rc < 0) return -1;
        if (!rc) continue;
        for (uint32_t at = s + 8u; at + 4u <= e - 4u; at += 4u) {
            const int prog = (b[at] << 8) | b[at + 1];
            if (prog != 0) { program = prog; pmt_pid = ((b[at + 2] & 0x1F) << 8) | b[at + 3]; break; }
        }
        if (pmt_pid < 0) return -1;
    }
    if (pmt_pid < 0) return -1;
    for (uint64_t p = 0; p < packets; ++p) {                     /* the first PMT section on that PID */
        const uint8_t* b = bytes + p * B + h;
        uint32_t s, e;
        const int rc = ts_section_in_packet(b, pmt_pid, 2u, 12u, &s, &e);
        if (rc < 0) return -1;
        if (!rc) continue;
        uint32_t at = s + 12u + (((b[s + 10] & 0x0Fu) << 8) | b[s + 11]);
        while (at + 5u <= e - 4u) {
            if ((int)b[at] == stream_type) {
                if (program_out) *program_out = program;
                return ((b[at + 1] & 0x1F) << 8) | b[at + 2];
            }
            at += 5u + (((b[at + 3] & 0x0Fu) << 8) | b[at + 4]);
        }
        return -1;
    }
    return -1;
}

#ifdef __HIPCC__
struct TsArgs {
    const uint8_t* ts; uint64_t n;                    /* the transport stream, bytes                                  */
    uint64_t packets; uint32_t B, lead; int pid;
    uint8_t* out; uint64_t out_cap;                   /* out NULL: plan only                                          */
    hbs_ts_pes* pes; uint64_t pes_cap;                /* nullable                                                     */
    hbs_summary* summary;
    /* scratch (lay_ts) */
    uint32_t* part;                                   /* 16 per block of kTsPacketsPerBlock packets (hbs_ts.hip)      */
    unsigned long long* ctl;                          /* 8: error, output bytes, PES packets, the first PES start's packet (~0: none) */
    hipEvent_t ev_begin, ev_end;
};
inline void lay_ts(Carver& w, TsArgs& a)
{
    const uint64_t blocks = (a.packets + kTsPacketsPerBlock - 1) / kTsPacketsPerBlock;
    a.part = w.take<uint32_t>(blocks * 64);
    a.ctl = w.take<unsigned long long>(64);
}
hipError_t launch_ts_demux(const TsArgs& a, hipStream_t st);
#endif

} // namespace hbs
#endif
