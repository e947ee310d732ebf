/*
 * hbs_mp4box.h -- what the MP4 headers share (ISO/IEC 14496-12): the big-endian reads and the box rule (mp4rd_box), host/device
 * inline functions that the kernels run too; and, host only, the one walk of a moov that the five init-segment calls make:
 * mp4_child finds a child box, mp4_resizable says whether a size can be patched in place, mp4_tkhd reads a trak's tkhd,
 * mp4_track_descend goes from a trak to the stsd entry that the caller's test chooses and leaves the seven boxes on the way in
 * an Mp4TrackPath.  Compiles with plain g++.
 */
#ifndef HBS_MP4BOX_H
#define HBS_MP4BOX_H

#include "hbs_common.h"

namespace hbs {

#define HBS_MP4_FOURCC(a, b, c, d) (((uint32_t)(a) << 24) | ((uint32_t)(b) << 16) | ((uint32_t)(c) << 8) | (uint32_t)(d))

/* the big-endian 32-bit word at p + at.  On the device p is 16-byte aligned and the word is put together from the one or two
 * aligned words that hold a byte of it: no load touches a 16-byte granule that holds no byte of the word.  On the host: four
 * byte loads, so that a sanitizer sees exactly the bytes that are read. */
HBS_HD uint32_t rd_be32(const uint8_t* p, uint64_t at)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t* w = reinterpret_cast<const uint32_t*>(p + (at & ~3ull));
    const uint32_t sh = (uint32_t)(at & 3u);
    const uint32_t lo = w[0], hi = sh ? w[1] : 0u;
    return __builtin_bswap32(alignbyte(hi, lo, sh));
#else
    return ((uint32_t)p[at] << 24) | ((uint32_t)p[at + 1] << 16) | ((uint32_t)p[at + 2] << 8) | (uint32_t)p[at + 3];
#endif
}
HBS_HD uint64_t rd_be64(const uint8_t* p, uint64_t at) { return ((uint64_t)rd_be32(p, at) << 32) | rd_be32(p, at + 4); }

/* the big-endian 16-bit value at p + at; on the device no load touches a granule that holds neither byte (rd_be32's way) */
HBS_HD uint32_t rd_be16(const uint8_t* p, uint64_t at)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t* w = reinterpret_cast<const uint32_t*>(p + (at & ~3ull));
    const uint32_t sh = (uint32_t)(at & 3u);
    const uint32_t lo = w[0], hi = sh == 3u ? w[1] : 0u;
    return __builtin_bswap32(alignbyte(hi, lo, sh)) >> 16;
#else
    return ((uint32_t)p[at] << 8) | (uint32_t)p[at + 1];
#endif
}

inline void wr_be32(uint8_t* q, uint32_t v) { q[0] = (uint8_t)(v >> 24); q[1] = (uint8_t)(v >> 16); q[2] = (uint8_t)(v >> 8); q[3] = (uint8_t)v; }   /* host only */

struct Mp4Box { uint64_t size; uint32_t type, head; };      /* head: 8, or 16 with a largesize */

/* the box at `at` in a container that ends at `end` (at < end <= the buffer's size); false: it breaks a size rule */
HBS_HD bool mp4rd_box(const uint8_t* p, uint64_t at, uint64_t end, Mp4Box& b)
{
    const uint64_t left = end - at;
    if (left < 8) return false;
    const uint32_t s = rd_be32(p, at);
    b.type = rd_be32(p, at + 4);
    b.head = 8; b.size = s;
    if (s == 1u) {
        if (left < 16) return false;
        b.size = rd_be64(p, at + 8); b.head = 16;
        if (b.size < 16) return false;
    } else if (s == 0u) b.size = left;
    else if (s < 8u) return false;
    return b.size <= left;
}

/* ---- host only: the walk to one track's sample entry ----------------------------------------------------------------------- */

/* where a box lies: p[pos, pos + head) its header, p[pay(), end()) its payload */
struct Mp4At { uint64_t pos, size; uint32_t head; uint64_t pay() const { return pos + head; } uint64_t end() const { return pos + size; } };

/* the first child of type `type` among the boxes that tile p[at, end).  1: c is it; 0: well-formed, none; -1: a box of the
 * container, in front of that child or (whole: the walk does not end at the child) behind it, breaks a size rule */
inline int mp4_child(const uint8_t* p, uint64_t at, uint64_t end, uint32_t type, Mp4At& c, bool whole = true)
{
    int found = 0;
    while (at < end) {
        Mp4Box b;
        if (!mp4rd_box(p, at, end, b)) return -1;
        if (b.type == type && !found) { c = Mp4At{at, b.size, b.head}; found = 1; if (!whole) break; }
        at += b.size;
    }
    return found;
}

/* the box can be resized in place: a size field of 0 ("to the end") or 1 (a 64-bit size) cannot */
inline bool mp4_resizable(const uint8_t* p, const Mp4At& b) { return b.head == 8u && rd_be32(p, b.pos) == b.size; }

struct Mp4Tkhd { uint32_t version, track_id, width, height; };     /* width, height: the integer parts */
/* the first tkhd among a trak's children p[at, end): version 0 or 1 and a payload that holds its fields */
inline bool mp4_tkhd(const uint8_t* p, uint64_t at, uint64_t end, Mp4Tkhd& k)
{
    Mp4At b;
    if (mp4_child(p, at, end, HBS_MP4_FOURCC('t', 'k', 'h', 'd'), b) <= 0 || b.size - b.head < 4) return false;
    const uint64_t a = b.pay();
    k.version = p[a];
    if (k.version > 1u || b.size - b.head < (k.version ? 96u : 84u)) return false;
    k.track_id = rd_be32(p, a + (k.version ? 20u : 12u));
    k.width = rd_be32(p, a + (k.version ? 88u : 76u)) >> 16; k.height = rd_be32(p, a + (k.version ? 92u : 80u)) >> 16;
    return true;
}

/* the seven boxes from the moov down to a track's sample entry */
enum : int { kPathMoov = 0, kPathTrak, kPathMdia, kPathMinf, kPathStbl, kPathStsd, kPathEntry, kPathBoxes };
struct Mp4TrackPath { Mp4At box[kPathBoxes]; };

/* From path.box[kPathTrak] down: mdia, minf, stbl, stsd, each the first of its type (whole: as mp4_child's); then the stsd's
 * entries one by one, at most entry_count of them, each held to the box rule when it is reached and handed to test(type, entry):
 * 1 it is the one (the walk ends: nothing behind that entry is looked at), 0 not it, -1 malformed.  Returns 1: path is filled
 * down to that entry; 0: no minf (path is filled down to the mdia) or no such entry; -1: malformed, or no mdia, stbl or stsd */
template <class Test>
inline int mp4_track_descend(const uint8_t* p, Mp4TrackPath& path, bool whole, Test&& test)
{
    const uint32_t kind[4] = {HBS_MP4_FOURCC('m', 'd', 'i', 'a'), HBS_MP4_FOURCC('m', 'i', 'n', 'f'), HBS_MP4_FOURCC('s', 't', 'b', 'l'), HBS_MP4_FOURCC('s', 't', 's', 'd')};
    for (int i = 0; i < 4; ++i) {
        const Mp4At& up = path.box[kPathTrak + i];
        const int rc = mp4_child(p, up.pay(), up.end(), kind[i], path.box[kPathMdia + i], whole);
        if (rc < 0) return -1;
        if (rc == 0) return i == 1 ? 0 : -1;                   /* (a trak without a minf is not ours; the other boxes are required) */
    }
    const Mp4At& stsd = path.box[kPathStsd];
    if (stsd.size - stsd.head < 8) return -1;
    const uint32_t entries = rd_be32(p, stsd.pay() + 4);
    uint64_t at = stsd.pay() + 8;
    for (uint32_t i = 0; i < entries && at < stsd.end(); ++i) {
        Mp4Box b;
        if (!mp4rd_box(p, at, stsd.end(), b)) return -1;
        path.box[kPathEntry] = Mp4At{at, b.size, b.head};
        const int rc = test(b.type, path.box[kPathEntry]);
        if (rc) return rc;
        at += b.size;
    }
    return 0;
}

} // namespace hbs
#endif
