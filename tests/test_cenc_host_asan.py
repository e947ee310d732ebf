"""The rules of hbs_cenc.h (cenc_expand_key, cenc_aes_block, cenc_ctr_*, cenc_nal_split, cenc_entries, cenc_entry,
cenc_nal_entries, cenc_sample_ok, cenc_range_begin) under AddressSanitizer and UBSan, in a stand-alone program: the block function,
and the plans of hbs_cenc.hip single-stepped on the host -- the subsample plan lane by lane over groups of kCencNalsPer NALs with
the run carried between them, the crypt plan range by range and tile by tile, window by window as the kernel's lanes go -- over
tables and data in exactly sized heap blocks.  The program prints counts and digests; tests/_cenc_ref.py must say the same of
every case.  Nothing is loaded into python."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import _cenc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "hevcbitstream_amd.h"
#include "hbs_cenc.h"

using namespace hbs;

static uint64_t digest(const uint8_t* p, uint64_t n)
{
    uint64_t h = 0;
    for (uint64_t i = 0; i < n; ++i) h = h * 1099511628211ull + p[i];
    return h;
}

template <class T> static T* block(FILE* f, uint64_t n)        /* a heap block of exactly n records, read from the file */
{
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    if (n && fread(p, sizeof(T), n, f) != n) exit(4);
    return p;
}

static void aes_case(FILE* f)
{
    uint8_t key[16], ctr[16];
    uint64_t n;
    if (fread(key, 16, 1, f) != 1 || fread(ctr, 16, 1, f) != 1 || fread(&n, 8, 1, f) != 1) exit(4);
    CencKey k;
    cenc_expand_key(key, k);
    const CencCtr c = cenc_ctr_load(ctr);
    uint8_t* out = (uint8_t*)malloc(n ? n * 16 : 1);
    for (uint64_t j = 0; j < n; ++j) {
        uint32_t in[4], ks[4];
        cenc_ctr_block(c, j, in);
        cenc_aes_block(k, in, ks, [](uint32_t x) { return cenc_te0(x); });
        for (uint32_t q = 0; q < 16; ++q) out[16 * j + q] = (uint8_t)cenc_block_byte(ks, q);
    }
    printf("aes %llu\n", (unsigned long long)digest(out, n * 16));
    free(out);
}

struct Lane { CencNal x[kCencNalsPer]; bool kept[kCencNalsPer], head[kCencNalsPer], last[kCencNalsPer], first[kCencNalsPer]; };

static void plan_case(FILE* f)
{
    hbs_cenc_plan_params prm;
    uint64_t hd[6];          /* stream bytes, NALs, AUs, keep given, payload offsets given, sub_cap */
    if (fread(&prm, 16, 1, f) != 1 || fread(hd, 8, 6, f) != 6) exit(4);
    const uint64_t n = hd[0], nn = hd[1], na = hd[2];
    uint8_t* src = block<uint8_t>(f, n);
    hbs_nal_entry* idx = block<hbs_nal_entry>(f, nn);
    uint32_t* au = block<uint32_t>(f, nn);
    uint8_t* keep = hd[3] ? block<uint8_t>(f, nn) : nullptr;
    uint64_t* po = hd[4] ? block<uint64_t>(f, nn) : nullptr;
    if (!cenc_plan_params_ok(&prm)) { printf("refused\n"); return; }
    const uint32_t L = (uint32_t)prm.length_size;
    const uint64_t lanes = (nn + kCencNalsPer - 1) / kCencNalsPer;
    std::vector<Lane> lane(lanes);
    uint64_t bad = 0, prev_end = 0, prot = 0, bytes = 0, kept_n = 0;
    bool tprev = false;
    /* k_cenc_runs: every NAL evaluated once */
    for (uint64_t k = 0; k < nn; ++k) {
        Lane& l = lane[k / kCencNalsPer];
        const int i = (int)(k % kCencNalsPer);
        const hbs_nal_entry e = idx[k];
        bool wrong = e.start > e.end || e.end > n || e.start < prev_end;
        bool kept = !wrong && (!keep || keep[k] != 0);
        if (kept && ((e.end - e.start) >> (8u * L)) != 0) { wrong = true; kept = false; }
        if (k != 0 && au[k] - au[k - 1] > 1u) wrong = true;
        if (k == nn - 1 && (uint64_t)(au[k] - au[0]) + 1 != na) wrong = true;
        l.first[i] = k == 0 || au[k] != au[k - 1];
        l.last[i] = k == nn - 1 || au[k + 1] != au[k];
        l.x[i].clear = l.x[i].protect = 0; l.x[i].bad = false;
        if (kept) {
            const uint32_t type = e.end > e.start ? ((uint32_t)src[e.start] >> 1) & 63u : 63u;
            l.x[i] = cenc_nal_split(L, e.start, e.end, type, po != nullptr, po ? po[k] : 0, prm.clear_lead, prm.flags);
            if (l.x[i].bad) { wrong = true; l.x[i].clear = l.x[i].protect = 0; }
            bytes += L + (e.end - e.start); kept_n += 1;
        }
        l.kept[i] = kept;
        l.head[i] = l.first[i] || tprev;
        tprev = l.x[i].protect != 0;
        if (wrong && !bad) bad = k + 1;
        prev_end = e.end;
    }
    if (bad) { printf("arg %llu\n", (unsigned long long)bad); goto done; }
    {
        /* k_cenc_carry .. k_cenc_place: the run a lane continues, the entries each NAL leaves, their places */
        std::vector<uint64_t> first(na + 1, 0);
        std::vector<hbs_cenc_subsample> sub;
        uint64_t run = 0;
        for (uint64_t k = 0; k < nn; ++k) {
            const Lane& l = lane[k / kCencNalsPer];
            const int i = (int)(k % kCencNalsPer);
            run = l.head[i] ? l.x[i].clear : run + l.x[i].clear;
            const uint64_t cnt = cenc_nal_entries(run, l.x[i].protect, l.last[i]);
            if (l.first[i]) first[au[k] - au[0]] = sub.size();
            for (uint64_t j = 0; j < cnt; ++j) sub.push_back(cenc_entry(run, l.x[i].protect, j, cnt));
            prot += l.x[i].protect;
        }
        first[na] = sub.size();
        printf("%s %llu %llu %llu %llu %llu %llu\n", sub.size() > hd[5] ? "cap" : "ok", (unsigned long long)sub.size(), (unsigned long long)prot,
               (unsigned long long)bytes, (unsigned long long)kept_n, (unsigned long long)digest((const uint8_t*)first.data(), (na + 1) * 8),
               (unsigned long long)digest((const uint8_t*)sub.data(), sub.size() * 8));
    }
done:
    free(src); free(idx); free(au); free(keep); free(po);
}

static void crypt_case(FILE* f)
{
    hbs_cenc_params prm;
    uint64_t hd[3];          /* data bytes, samples, entries in the table */
    if (fread(&prm, 48, 1, f) != 1 || fread(hd, 8, 3, f) != 3) exit(4);
    const uint64_t n = hd[0], ns = hd[1];
    uint8_t* data = block<uint8_t>(f, n);
    uint64_t* off = block<uint64_t>(f, ns);
    uint64_t* size = block<uint64_t>(f, ns);
    uint64_t* first = block<uint64_t>(f, ns + 1);
    hbs_cenc_subsample* sub = block<hbs_cenc_subsample>(f, hd[2]);
    uint8_t* iv = block<uint8_t>(f, ns * 16);
    if (!cenc_params_ok(&prm)) { printf("refused\n"); return; }
    CencKey key;
    cenc_expand_key(prm.key, key);
    const uint64_t iv_base = cenc_be64(prm.iv0);
    uint64_t bad = 0;
    /* k_cenc_samples, k_cenc_begin */
    for (uint64_t s = 0; s < ns && !bad; ++s)
        if (!cenc_sample_ok(s, off[s], size[s], s + 1 < ns, s + 1 < ns ? off[s + 1] : 0, n, first[s], first[s + 1])) bad = s + 1;
    const uint64_t E = (bad || !ns) ? 0 : first[ns];
    /* k_cenc_range_sum, k_cenc_range_scan */
    std::vector<uint64_t> rB(kCencRanges + 1, 0), rK(kCencRanges + 1, 0);
    for (uint32_t g = 0; g < kCencRanges; ++g) {
        uint64_t b = 0, k = 0;
        for (uint64_t e = cenc_range_begin(E, g, kCencRanges); e < cenc_range_begin(E, g + 1, kCencRanges); ++e) {
            b += (uint64_t)sub[e].clear + sub[e].protect; k += sub[e].protect;
            if (sub[e].clear > kCencMaxClear) {
                uint64_t s = 0;
                while (s + 1 < ns && first[s + 1] <= e) s += 1;
                if (!bad || s + 1 < bad) bad = s + 1;
            }
        }
        rB[g + 1] = rB[g] + b; rK[g + 1] = rK[g] + k;
    }
    const uint64_t all = rK[kCencRanges];
    /* k_cenc_at, k_cenc_sizes */
    std::vector<uint64_t> at_b(ns + 1, 0), at_k(ns + 1, 0);
    if (!bad) {
        for (uint32_t g = 0; g < kCencRanges; ++g) {
            uint64_t b = rB[g], k = rK[g];
            const uint64_t lo = cenc_range_begin(E, g, kCencRanges), hi = cenc_range_begin(E, g + 1, kCencRanges);
            for (uint64_t e = lo; e <= hi; ++e) {
                if (e < hi || e == E)
                    for (uint64_t s = 0; s <= ns; ++s) if (first[s] == e) { at_b[s] = b; at_k[s] = k; }
                if (e < hi) { b += (uint64_t)sub[e].clear + sub[e].protect; k += sub[e].protect; }
            }
        }
        for (uint64_t s = 0; s < ns && !bad; ++s) if (at_b[s + 1] - at_b[s] != size[s]) bad = s + 1;
    }
    if (bad) { printf("arg %llu\n", (unsigned long long)bad); }
    else {
        /* k_cenc_iv, k_cenc_crypt */
        if (prm.iv_mode) for (uint64_t s = 0; s < ns; ++s) cenc_ctr_store(cenc_ctr_seq(iv_base, s), iv + 16 * s);
        const uint64_t lasts = ns - 1;
        for (uint64_t t0 = 0; t0 < all; t0 += kCencTileBytes) {
            const uint64_t t1 = all - t0 < kCencTileBytes ? all : t0 + kCencTileBytes;
            uint32_t g = 0;
            while (g + 1 < kCencRanges && rK[g + 1] <= t0) g += 1;
            uint64_t e = cenc_range_begin(E, g, kCencRanges), Bc = rB[g], Kc = rK[g];
            while (e < E && Kc < t1) {
                const uint32_t cnt = E - e < 256 ? (uint32_t)(E - e) : 256u;
                uint64_t sk[257], sp[256];
                uint64_t b = Bc, k = Kc;
                for (uint32_t i = 0; i < cnt; ++i) { sk[i] = k; sp[i] = b + sub[e + i].clear; b += (uint64_t)sub[e + i].clear + sub[e + i].protect; k += sub[e + i].protect; }
                sk[cnt] = k;
                const uint64_t Kend = k;
                if (Kend > t0) for (uint32_t lane = 0; lane < 256; ++lane) {
                    uint64_t s = 0;
                    for (uint64_t w = t0 + 16u * lane; w < t1; w += 16u * 256u) {
                        const uint64_t wend = w + 16u < t1 ? w + 16u : t1;
                        while (s < lasts && at_k[s + 1] <= w) s += 1;
                        uint64_t bb = at_k[s] + ((w - at_k[s] + 15u) & ~15ull);
                        for (;;) {
                            const uint64_t send = at_k[s + 1];
                            if (bb < send && bb < wend && bb >= Kc && bb < Kend) {
                                const uint32_t len = send - bb < 16u ? (uint32_t)(send - bb) : 16u;
                                uint32_t in[4], ks[4];
                                const CencCtr c = prm.iv_mode ? cenc_ctr_seq(iv_base, s) : cenc_ctr_load(iv + 16 * s);
                                cenc_ctr_block(c, (bb - at_k[s]) >> 4, in);
                                cenc_aes_block(key, in, ks, [](uint32_t x) { return cenc_te0(x); });
                                uint32_t i = 0;
                                while (i + 1 < cnt && sk[i + 1] <= bb) i += 1;
                                uint64_t pos = off[s] - at_b[s] + sp[i] + (bb - sk[i]), rem = sk[i + 1] - bb, ent = e + i;
                                uint32_t q = 0;
                                while (q < len) {
                                    if (rem == 0) { ent += 1; pos += sub[ent].clear; rem = sub[ent].protect; continue; }
                                    data[pos] = (uint8_t)(data[pos] ^ cenc_block_byte(ks, q));
                                    pos += 1; rem -= 1; q += 1;
                                }
                            }
                            if (send >= wend || s == lasts) break;
                            s += 1;
                            while (s < lasts && at_k[s + 1] <= send) s += 1;
                            bb = at_k[s];
                            if (bb >= wend) break;
                        }
                    }
                }
                e += cnt; Kc = Kend; Bc = b;
            }
        }
        printf("ok %llu %llu %llu %llu\n", (unsigned long long)E, (unsigned long long)all, (unsigned long long)digest(data, n),
               (unsigned long long)digest(iv, ns * 16));
    }
    free(data); free(off); free(size); free(first); free(sub); free(iv);
}

int main(int argc, char** argv)
{
    static_assert(sizeof(hbs_cenc_plan_params) == 16 && sizeof(hbs_cenc_params) == 48 && sizeof(hbs_cenc_subsample) == 8 && sizeof(hbs_nal_entry) == 32, "layouts");
    FILE* f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    if (!f) return 3;
    for (;;) {
        const int kind = fgetc(f);
        if (kind == EOF) break;
        if (kind == 'A') aes_case(f);
        else if (kind == 'S') plan_case(f);
        else if (kind == 'C') crypt_case(f);
        else return 5;
    }
    fclose(f);
    return 0;
}
"""

NAL_ENTRY = np.dtype([("start", "<u8"), ("end", "<u8"), ("rbsp_off", "<u8"), ("rbsp_len", "<u4"), ("status", "<i4")])
PLAN_PARAMS = np.dtype([("length_size", "<i4"), ("flags", "<u4"), ("clear_lead", "<u4"), ("reserved", "<u4")])
PARAMS = np.dtype([("key", "u1", (16,)), ("iv0", "u1", (16,)), ("scheme", "<u4"), ("iv_mode", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])


def digest(raw):
    h = 0
    for v in bytes(raw):
        h = (h * 1099511628211 + v) & R.M64
    return h


def make_stream(rng, n_nals, sizes=None, big=()):
    """a stream of NALs with 3-byte gaps: (stream, starts, ends, nal_au, n_aus, payload_off)"""
    types = rng.choice([1, 19, 32, 33, 34, 39, 35], n_nals)
    sizes = rng.integers(0, 90, n_nals) if sizes is None else np.array(sizes)
    for k, z in big:
        sizes[k], types[k] = z, 39
    sizes[(types < 32) & (sizes == 1)] = 2                    # a slice of one byte has no payload offset the call accepts
    starts =np.cumsum(sizes + 3) - sizes
    ends = starts + sizes
    stream = rng.integers(0, 256, int(ends[-1]) + 5 if n_nals else 5, dtype=np.uint8)
    for k in range(n_nals):
        if sizes[k]:
            stream[starts[k]] = (types[k] << 1) | (stream[starts[k]] & 0x81)
    nal_au = (np.cumsum(rng.integers(0, 2, n_nals)) + 5).astype(np.uint32) if n_nals else np.zeros(0, dtype=np.uint32)
    n_aus = int(nal_au[-1] - nal_au[0]) + 1 if n_nals else 0
    po = np.full(n_nals, R.M64, dtype=np.uint64)
    for k in range(n_nals):
        if types[k] < 32 and sizes[k] >= 2:
            po[k] = starts[k] + rng.integers(2, sizes[k] + 1)
    return stream, starts.astype(np.uint64), ends.astype(np.uint64), nal_au, n_aus, po


def plan_cases():
    rng = np.random.default_rng(2301)
    out = []
    for n_nals, L, flags, lead, use_keep, use_po in ((0, 4, 0, 96, False, False), (1, 4, 0, 2, False, False), (7, 1, 0, 2, True, True), (8, 2, 1, 5, True, True),
                                                     (9, 4, 1, 96, False, True), (300, 4, 0, 2, True, True), (300, 1, 1, 96, True, False), (700, 2, 0, 7, True, True)):
        big = ((3, 70000), (n_nals - 2, 131070 - 4)) if n_nals >= 300 and L == 4 else ()
        stream, starts, ends, nal_au, n_aus, po = make_stream(rng, n_nals, big=big)
        keep = (rng.integers(0, 4, n_nals) > 0).astype(np.uint8) if use_keep else None
        out.append(dict(stream=stream, starts=starts, ends=ends, nal_au=nal_au, n_aus=n_aus, L=L, flags=flags, clear_lead=lead, keep=keep,
                        payload_off=po if use_po else None, sub_cap=1 << 40))
    # errors: a payload offset the parse did not give, one short, one long; an index out of order; capacity
    base = out[5]
    vcl = [k for k in range(300) if base["payload_off"][k] != R.M64 and base["keep"][k]]
    for value in (lambda k: R.M64, lambda k: int(base["starts"][k]) + 1, lambda k: int(base["ends"][k]) + 1):
        c = dict(base)
        c["payload_off"] = base["payload_off"].copy()
        c["payload_off"][vcl[3]] = value(vcl[3])
        out.append(c)
    c = dict(base)
    c["starts"] = base["starts"].copy()
    c["starts"][17] = base["ends"][16] - 1
    out.append(c)
    c = dict(base)
    c["sub_cap"] = 5
    out.append(c)
    return out


def plan_record(c):
    n = len(c["starts"])
    idx = np.zeros(n, dtype=NAL_ENTRY)
    idx["start"], idx["end"] = c["starts"], c["ends"]
    prm = np.zeros(1, dtype=PLAN_PARAMS)
    prm[0] = (c["L"], c["flags"], c["clear_lead"], 0)
    raw = b"S" + prm.tobytes() + struct.pack("<6Q", len(c["stream"]), n, c["n_aus"], c["keep"] is not None, c["payload_off"] is not None, c["sub_cap"])
    raw += c["stream"].tobytes() + idx.tobytes() + c["nal_au"].tobytes()
    if c["keep"] is not None:
        raw += c["keep"].tobytes()
    if c["payload_off"] is not None:
        raw += c["payload_off"].tobytes()
    return raw


def plan_want(c):
    r = R.subsamples(c["stream"], c["starts"].astype(np.int64), c["ends"].astype(np.int64), c["nal_au"], c["n_aus"], c["L"], keep=c["keep"],
                     payload_off=c["payload_off"], flags=c["flags"], clear_lead=c["clear_lead"], sub_cap=c["sub_cap"])
    if r["error"] == R.E_ARG:
        return "arg %d" % r["bad"]
    return "%s %d %d %d %d %d %d" % ("cap" if r["error"] else "ok", len(r["sub"]), r["protected"], r["sample_bytes"], r["kept"],
                                     digest(r["sub_first"].tobytes()), digest(r["sub"].tobytes()))


def make_samples(rng, n_samples, extra=()):
    """samples with random gaps and 0..6 entries each, then the `extra` lists of entries: (data_bytes, off, size, first, sub)"""
    subs, first, off, size, at = [], [0], [], [], int(rng.integers(0, 40))
    for s in range(n_samples + len(extra)):
        if s < n_samples:
            e = [(int(rng.integers(0, 120)) if rng.integers(0, 3) else 0, int(rng.integers(0, 100)) if rng.integers(0, 4) else 0)
                 for _ in range(int(rng.integers(0, 7)))]
        else:
            e = list(extra[s - n_samples])
        z = sum(a + b for a, b in e)
        subs += e
        first.append(len(subs))
        off.append(at)
        size.append(z)
        at += z + int(rng.integers(0, 30))
    return (at + 7, np.array(off, dtype=np.uint64), np.array(size, dtype=np.uint64), np.array(first, dtype=np.uint64),
            np.array(subs, dtype=R.SUBSAMPLE).reshape(-1))


def crypt_cases():
    rng = np.random.default_rng(2302)
    out = []
    straddle = [(5, 7), (3, 30), (0, 1), (65535, 0), (2, 11), (0, 0), (1, 16)]
    many = [(int(rng.integers(0, 9)), int(rng.integers(0, 40))) for _ in range(1500)]
    for n_samples, extra, mode in ((0, (), 1), (1, (), 0), (0, (straddle,), 0), (40, (straddle,), 1), (300, ([(9, 200001)], many), 0), (5, (), 1)):
        n, off, size, first, sub = make_samples(rng, n_samples, extra)
        out.append(dict(n=n, off=off, size=size, first=first, sub=sub, mode=mode, data=rng.integers(0, 256, n, dtype=np.uint8),
                        key=bytes(rng.integers(0, 256, 16, dtype=np.uint8)), iv0=bytes([0xFF] * 7 + [0xFE]) + bytes(rng.integers(0, 256, 8, dtype=np.uint8)),
                        iv=rng.integers(0, 256, 16 * len(off), dtype=np.uint8)))
    out[1]["iv"][8:16] = 0xFF                                             # the counter wraps inside the sample
    base = out[3]
    for change in ("short", "overlap", "past", "clear", "first"):
        c = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
        if change == "short":
            c["size"][11] += 1
        elif change == "overlap":
            c["off"][20] = c["off"][19]
            c["size"][19] = max(int(c["size"][19]), 1)
        elif change == "past":
            c["n"] = int(c["off"][-1] + c["size"][-1]) - 1
            c["data"] = c["data"][: c["n"]]
        elif change == "clear":
            e = int(c["first"][40])
            c["sub"][e + 3] = (65536, 0)
        else:
            c["first"][7] = c["first"][8] + 1
        out.append(c)
    return out


def crypt_record(c):
    prm = np.zeros(1, dtype=PARAMS)
    prm["key"][0] = np.frombuffer(c["key"], dtype=np.uint8)
    prm["iv0"][0] = np.frombuffer(c["iv0"], dtype=np.uint8)
    prm["scheme"], prm["iv_mode"] = R.SCHEME_CENC, c["mode"]
    return (b"C" + prm.tobytes() + struct.pack("<3Q", c["n"], len(c["off"]), len(c["sub"])) + c["data"].tobytes() + c["off"].tobytes() +
            c["size"].tobytes() + c["first"].tobytes() + c["sub"].tobytes() + c["iv"].tobytes())


def crypt_want(c):
    bad = R.crypt_check(c["n"], c["off"], c["size"], c["first"], c["sub"])
    if bad:
        return "arg %d" % bad
    data, done, used = R.crypt(c["data"], c["off"], c["size"], c["first"], c["sub"], c["key"], iv=c["iv"] if c["mode"] == 0 else None,
                               iv0=c["iv0"] if c["mode"] else None)
    return "ok %d %d %d %d" % (len(c["sub"]), done, digest(data.tobytes()), digest(used.tobytes()))


def aes_cases():
    return [(bytes(range(16)), bytes.fromhex("00112233445566778899aabbccddeeff"), 1),
            (bytes.fromhex("2b7e151628aed2a6abf7158809cf4f3c"), bytes.fromhex("f0f1f2f3f4f5f6f7f8f9fafbfcfdfeff"), 4),
            (bytes.fromhex("2b7e151628aed2a6abf7158809cf4f3c"), bytes.fromhex("00000000000000" "01" + "ff" * 8), 2), (bytes(16), bytes(16), 0)]


def test_plans_and_block_function_single_stepped_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no g++")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
             "-static-libasan", "-static-libubsan"]
    # whether the compiler has the sanitizer runtimes is asked of a program that includes nothing of the project's ...
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    probed = subprocess.run([cxx] + flags + ["-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True)
    if probed.returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime: " + (probed.stderr.strip().splitlines() or ["?"])[-1])
    # ... so that the real program failing to build is a failure, whatever the compiler says
    src = tmp_path / "cenc_host_asan.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "cenc_host_asan"
    cmd = [cxx] + flags + ["-I", os.path.join(ROOT, "hevcbitstream_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    want = []
    with open(tmp_path / "cases.bin", "wb") as f:
        for key, ctr, n in aes_cases():
            f.write(b"A" + key + ctr + struct.pack("<Q", n))
            want.append("aes %d" % digest(R.keystream(key, ctr, 16 * n).tobytes()))
        for c in plan_cases():
            f.write(plan_record(c))
            want.append(plan_want(c))
        for c in crypt_cases():
            f.write(crypt_record(c))
            want.append(crypt_want(c))
    run = subprocess.run([str(exe), str(tmp_path / "cases.bin")], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-6000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(want)
    for i, (got, exp) in enumerate(zip(lines, want)):
        assert got == exp, i
    assert {ln.split()[0] for ln in lines} == {"aes", "ok", "arg", "cap"}
    assert want[0] == "aes %d" % digest(bytes.fromhex("69c4e0d86a7b0430d8cdb78070b4c55a"))
