/* hbs_rtpbytes.h -- device-only: how the kernels of hbs_rtp_unpack (hbs_rtpun.hip) and hbs_rtp_order (hbs_rtpord.hip) read a
 * packet of the table -- its first 16 bytes from one or two aligned 16-byte loads, which covers the fixed header, the PayloadHdr
 * and the FU header of a packet without CSRC entries; more bytes are read one by one.  No load touches a 16-byte granule that
 * holds no byte of the packet. */
#ifndef HBS_RTPBYTES_H
#define HBS_RTPBYTES_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hbs_wave.h"

namespace hbs {

/* a packet's bytes: the first 16 in registers, the others in memory */
struct PacketBytes {
    const uint8_t* p;
    uint64_t lo, hi;
    __device__ __forceinline__ uint32_t operator()(uint64_t i) const
    {
        if (i < 8) return (uint32_t)(lo >> (8u * (uint32_t)i)) & 0xFFu;
        if (i < 16) return (uint32_t)(hi >> (8u * (uint32_t)(i - 8))) & 0xFFu;
        return p[i];
    }
};

__device__ __forceinline__ uint64_t funnel(uint64_t lo, uint64_t hi, uint32_t bits) { return bits ? (lo >> bits) | (hi << (64u - bits)) : lo; }

/* the packet d_in[off, off + size), size > 0, inside the input: its first bytes from the aligned 16-byte granule that holds its
 * first byte and, when that one holds bytes of the packet as well, the next */
__device__ __forceinline__ PacketBytes load_packet(const uint8_t* src, uint64_t off, uint64_t size)
{
    const uint64_t g = off & ~15ull;
    const uint32_t sh = (uint32_t)(off & 15u);
    const u32x4 a = *reinterpret_cast<const u32x4*>(src + g);
    u32x4 b;
    b.x = b.y = b.z = b.w = 0;
    if (g + 16 < off + size) b = *reinterpret_cast<const u32x4*>(src + g + 16);
    const uint64_t w0 = a.x | ((uint64_t)a.y << 32), w1 = a.z | ((uint64_t)a.w << 32);
    const uint64_t w2 = b.x | ((uint64_t)b.y << 32), w3 = b.z | ((uint64_t)b.w << 32);
    const bool up = sh >= 8;
    const uint32_t r = 8u * (sh & 7u);
    PacketBytes pb;
    pb.p = src + off;
    pb.lo = funnel(up ? w1 : w0, up ? w2 : w1, r);
    pb.hi = funnel(up ? w2 : w1, up ? w3 : w2, r);
    return pb;
}

} // namespace hbs
#endif
