"""The host/device rules of hbs_mp4stblw.h (stblw_lane, stblw_chunk_start, stblw_run_start, stblw_stsz_constant, stblw_layout ...)
and hbs_mp4_moov_host under AddressSanitizer and UBSan, in a stand-alone program: hbs_mp4_stbl_write as a plain host loop over
the rule functions, on tables in exactly sized heap blocks and into an output of exactly T bytes -- random tracks, every sample
error, N = 0, a capacity one byte short -- and the moov writer into outputs of exactly the bytes it asks for, with `cap` cut at
every length.  The program prints a verdict and a digest per case; tests/_mp4_stbl_write_ref.py must say the same.  Nothing is
loaded into python."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import _mp4_stbl_write_ref as Wr
from tests.test_mp4_read_ref import NALS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "hevcbitstream_amd.h"
#include "hbs_mp4stblw.h"

static uint64_t h;
static void mix(uint64_t v) { h = h * 1099511628211ull + v; }
typedef unsigned long long ull;

static void put32(uint8_t* out, uint64_t at, uint32_t v)
{
    out[at] = (uint8_t)(v >> 24); out[at + 1] = (uint8_t)(v >> 16); out[at + 2] = (uint8_t)(v >> 8); out[at + 3] = (uint8_t)v;
}

/* hbs_mp4_stbl_write on the host: one loop over the samples, one over the chunks, one over the runs */
static void write(const hbs::StblwIn& in, const hbs_mp4_stbl_write_params& prm, bool plan, uint64_t out_cap)
{
    using namespace hbs;
    const uint64_t N = in.n;
    const bool co64 = (prm.flags & HBS_MP4_STBL_CO64) != 0;
    std::vector<uint64_t> chunk_first, stts_first, ctts_first, sync;
    uint64_t s = 0, bytes = 0, dur = 0, differ = 0, neg = 0, bad = 0;
    for (uint64_t k = 0; k < N; ++k) {
        StblwLane l;
        stblw_lane(in, k, l);
        if (l.brk) s = k;
        const bool chunk = stblw_chunk_start(k, s, prm.max_chunk_samples);
        if ((l.bad || (chunk && !stblw_chunk_off_ok(l.o, co64))) && !bad) bad = k + 1;
        if (chunk) chunk_first.push_back(k);
        if (l.stts_run) stts_first.push_back(k);
        if (l.ctts_run) ctts_first.push_back(k);
        if (l.sync) sync.push_back(k);
        bytes += l.z; dur += l.delta; differ += l.z != in.size[0]; neg += l.cts < 0;
    }
    if (bad) { printf("sample %llu\n", (ull)(bad - 1)); return; }
    const uint64_t C = chunk_first.size(), T = stts_first.size(), K = ctts_first.size();
    auto len = [&](uint64_t c) { return (c + 1 < C ? chunk_first[c + 1] : N) - chunk_first[c]; };
    std::vector<uint64_t> stsc;
    for (uint64_t c = 0; c < C; ++c) if (stblw_run_start(c, len(c), c ? len(c - 1) : 0)) stsc.push_back(c);
    const bool constant = stblw_stsz_constant(N, differ, N ? in.size[0] : 0);
    const uint64_t entries[kSwBoxes] = {T, K, sync.size(), stsc.size(), N, C};
    uint64_t off[kSwBoxes], size[kSwBoxes], total;
    const uint32_t box = stblw_layout(entries, in.pts != nullptr, in.sflags != nullptr, constant, co64, off, size, total);
    if (box) { printf("box %u\n", box - 1); return; }
    if (total > mp4_stbl_write_bytes(N, in.pts != nullptr, in.sflags != nullptr, prm.flags)) { printf("bound\n"); return; }
    if (plan) { printf("plan %llu %llu %llu %llu %llu\n", (ull)N, (ull)C, (ull)bytes, (ull)total, (ull)dur); return; }
    if (out_cap < total) { printf("capacity %llu %llu %llu %llu %llu\n", (ull)N, (ull)C, (ull)bytes, (ull)total, (ull)dur); return; }
    uint8_t* out = (uint8_t*)malloc(total ? total : 1);        /* a heap block of exactly T bytes */
    memset(out, 0xA5, total);
    for (int b = 0; b < kSwBoxes; ++b) {
        if (!size[b]) continue;
        uint64_t at = off[b];
        put32(out, at, (uint32_t)size[b]); put32(out, at + 4, stblw_fourcc(b, co64)); put32(out, at + 8, b == kSwCtts && neg ? 0x01000000u : 0u);
        at += 12;
        if (b == kSwStsz) { put32(out, at, constant ? (uint32_t)in.size[0] : 0u); at += 4; }
        put32(out, at, (uint32_t)entries[b]);
    }
    for (uint64_t i = 0; i < T; ++i) {
        uint64_t t, delta;
        stblw_times(in, stts_first[i], t, delta);
        put32(out, off[kSwStts] + 16 + i * 8, (uint32_t)((i + 1 < T ? stts_first[i + 1] : N) - stts_first[i]));
        put32(out, off[kSwStts] + 20 + i * 8, (uint32_t)delta);
    }
    for (uint64_t i = 0; i < K; ++i) {
        uint64_t t, delta;
        int64_t cts;
        stblw_times(in, ctts_first[i], t, delta);
        stblw_cts(in.pts[ctts_first[i]], t, cts);
        put32(out, off[kSwCtts] + 16 + i * 8, (uint32_t)((i + 1 < K ? ctts_first[i + 1] : N) - ctts_first[i]));
        put32(out, off[kSwCtts] + 20 + i * 8, (uint32_t)(int32_t)cts);
    }
    for (uint64_t i = 0; i < sync.size(); ++i) put32(out, off[kSwStss] + 16 + i * 4, (uint32_t)(sync[i] + 1));
    for (uint64_t i = 0; i < stsc.size(); ++i) {
        put32(out, off[kSwStsc] + 16 + i * 12, (uint32_t)(stsc[i] + 1)); put32(out, off[kSwStsc] + 20 + i * 12, (uint32_t)len(stsc[i]));
        put32(out, off[kSwStsc] + 24 + i * 12, 1);
    }
    if (!constant) for (uint64_t k = 0; k < N; ++k) put32(out, off[kSwStsz] + 20 + k * 4, (uint32_t)in.size[k]);
    for (uint64_t c = 0; c < C; ++c) {
        const uint64_t o = in.off[chunk_first[c]] + in.data_offset;
        if (co64) { put32(out, off[kSwStco] + 16 + c * 8, (uint32_t)(o >> 32)); put32(out, off[kSwStco] + 20 + c * 8, (uint32_t)o); }
        else put32(out, off[kSwStco] + 16 + c * 4, (uint32_t)o);
    }
    h = 0;
    for (uint64_t i = 0; i < total; i += 4) mix(((uint32_t)out[i] << 24) | (out[i + 1] << 16) | (out[i + 2] << 8) | out[i + 3]);
    for (int b = 0; b < kSwBoxes; ++b) { mix(size[b] ? off[b] + 8 : 0); mix(size[b] ? size[b] - 8 : 0); }
    free(out);
    printf("ok %llu %llu %llu %llu %llu %llu\n", (ull)N, (ull)C, (ull)bytes, (ull)total, (ull)dur, (ull)h);
}

/* hbs_mp4_moov_host with `cap` cut at every length, each time into a heap block of exactly cap bytes */
static void moov(const hbs_mp4_init_params& p, int flags, const std::vector<std::vector<uint8_t>>& nals, uint64_t duration, uint64_t tables_bytes)
{
    std::vector<const uint8_t*> ptr;
    std::vector<uint64_t> len;
    for (auto& x : nals) { ptr.push_back(x.data()); len.push_back(x.size()); }
    const int64_t need = hbs::mp4_moov_host(&p, flags, ptr.data(), len.data(), ptr.size(), duration, tables_bytes, nullptr, 0);
    if (need < 0) { printf("refused\n"); return; }
    for (int64_t cap = 0; cap <= need; ++cap) {
        uint8_t* out = (uint8_t*)malloc(cap ? cap : 1);
        memset(out, 0x5A, cap);
        if (hbs::mp4_moov_host(&p, flags, ptr.data(), len.data(), ptr.size(), duration, tables_bytes, out, (uint64_t)cap) != need) { printf("moved\n"); return; }
        if (cap < need) { for (int64_t i = 0; i < cap; ++i) if (out[i] != 0x5A) { printf("touched\n"); return; } }
        else { h = 0; for (int64_t i = 0; i < need; ++i) mix(out[i]); }
        free(out);
    }
    printf("moov %lld %llu\n", (long long)need, (ull)h);
}

/* what no table of a testable size reaches: the 2^62 bounds, deltas at 0 and 2^32 - 1, cts at +-2^31, the 2^32 box size rule */
static int limits()
{
    using namespace hbs;
    const uint64_t L = 1ull << 62, M = 0xFFFFFFFFull;
    uint64_t o, t, d;
    int64_t c;
    int bad = 0;
    bad |= !stblw_place(L - 2, 1, 0, o) || o != L - 2 || stblw_place(L - 1, 1, 0, o) || stblw_place(L, 0, 0, o) || !stblw_place(L - 1, 0, 0, o);
    bad |= !stblw_place(0, M, L - 1 - M, o) || stblw_place(0, M, L - M, o) || stblw_place(0, M + 1, 0, o) || stblw_place(~0ull, 0, 1, o);
    bad |= stblw_place(~0ull - 5, 0, L - 1, o) || !stblw_place(5, 5, L - 11, o) || o != L - 6;
    bad |= !stblw_chunk_off_ok(M, false) || stblw_chunk_off_ok(M + 1, false) || !stblw_chunk_off_ok(L, true);
    bad |= !stblw_contiguous(5, 3, 8) || stblw_contiguous(5, 3, 9) || stblw_contiguous(~0ull, 1, 0) || !stblw_contiguous(~0ull, 0, ~0ull);
    bad |= !stblw_chunk_start(7, 7, 0) || stblw_chunk_start(8, 7, 0) || !stblw_chunk_start(10, 7, 3) || stblw_chunk_start(9, 7, 3) || !stblw_chunk_start(9, 7, 1);
    bad |= !stblw_chunk_start(M, 0, (uint32_t)M) || stblw_chunk_start(M - 1, 0, (uint32_t)M);
    const uint64_t two[2] = {L - 1, L};
    bad |= !stblw_dts(two, 0, 0, 0, t) || t != L - 1 || stblw_dts(two, 0, 0, 1, t);
    bad |= !stblw_dts(nullptr, L - 1, 7, 0, t) || t != L - 1 || stblw_dts(nullptr, L - 1, 1, 1, t) || !stblw_dts(nullptr, L - 1 - (1ull << 29) * M, (uint32_t)M, 1ull << 29, t) || t != L - 1;
    bad |= stblw_dts(nullptr, L - (1ull << 29) * M, (uint32_t)M, 1ull << 29, t) || stblw_dts(nullptr, L - 1, (uint32_t)M, M, t);
    bad |= !stblw_delta(false, 5, 5, 9, d) || d != 0 || !stblw_delta(false, 5, 5 + M, 9, d) || d != M || stblw_delta(false, 5, 6 + M, 9, d);
    bad |= stblw_delta(false, 5, 4, 9, d) || !stblw_delta(true, 5, 4, 9, d) || d != 9 || stblw_delta(false, 0, ~0ull, 9, d) || stblw_delta(false, ~0ull, 0, 9, d);
    bad |= !stblw_cts((1ull << 31) - 1, 0, c) || c != 2147483647ll || stblw_cts(1ull << 31, 0, c) || !stblw_cts(0, 1ull << 31, c) || c != -2147483648ll;
    bad |= stblw_cts(0, (1ull << 31) + 1, c) || stblw_cts(L, L - 1, c) || stblw_cts(L - 1, L, c) || !stblw_cts(L - 1, L - 1, c) || c != 0;
    bad |= stblw_cts(0, ~0ull, c) || stblw_cts(~0ull, 0, c);
    bad |= !stblw_run_start(0, 1, 1) || stblw_run_start(1, 1, 1) || !stblw_run_start(1, 1, 2);
    bad |= !stblw_stsz_constant(1, 0, 5) || stblw_stsz_constant(0, 0, 5) || stblw_stsz_constant(3, 1, 5) || stblw_stsz_constant(3, 0, 0);
    bad |= !stblw_sync(0x02000000u) || stblw_sync(0x01010000u);
    /* the box size rule: the largest count whose box has 32 bits of size, and one more, box by box */
    const uint64_t most[kSwBoxes] = {(M - 16) / 8, (M - 16) / 8, (M - 16) / 4, (M - 16) / 12, (M - 20) / 4, (M - 16) / 8};
    for (int b = 0; b < kSwBoxes; ++b) {
        uint64_t e[kSwBoxes] = {1, 1, 1, 1, 1, 1}, off[kSwBoxes], size[kSwBoxes], total;
        e[b] = most[b];
        bad |= stblw_layout(e, true, true, false, true, off, size, total) != 0 || size[b] > M || size[b] + 12 <= M || total % 4 != 0;
        e[b] = most[b] + 1;
        bad |= stblw_layout(e, true, true, false, true, off, size, total) != 1u + (uint32_t)b;
        if (b == kSwCtts || b == kSwStss) bad |= stblw_layout(e, false, false, false, true, off, size, total) != 0 || size[b] != 0;
    }
    uint64_t e[kSwBoxes] = {M, M, M, M, M, M}, off[kSwBoxes], size[kSwBoxes], total;
    bad |= stblw_layout(e, true, true, false, false, off, size, total) != 1u + kSwStts || stblw_layout(e, false, true, true, false, off, size, total) != 1u + kSwStts;
    e[kSwStts] = 1; e[kSwStsc] = 1; e[kSwStss] = 1; e[kSwStco] = (M - 16) / 4;
    bad |= stblw_layout(e, false, true, true, false, off, size, total) != 0 || size[kSwStsz] != 20 || size[kSwStco] != 16 + 4 * ((M - 16) / 4) || off[kSwStco] != 24 + 20 + 28 + 20;
    bad |= stblw_layout(e, false, true, true, true, off, size, total) != 1u + kSwStco || stblw_layout(e, false, true, false, false, off, size, total) != 1u + kSwStsz;
    bad |= mp4_stbl_write_bytes(M, 1, 1, 1) != 100 + 44 * M || mp4_stbl_write_bytes(M + 1, 1, 1, 1) != 0 || mp4_stbl_write_bytes(0, 0, 0, 0) != 68;
    return bad;
}

int main(int argc, char** argv)
{
    static_assert(sizeof(hbs_mp4_stbl_write_params) == 32, "hbs_mp4_stbl_write_params");
    if (limits()) return 5;
    FILE* f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    if (!f) return 3;
    for (;;) {
        uint32_t head[2];
        uint64_t n, arg;
        if (fread(head, 4, 2, f) != 2 || fread(&n, 8, 1, f) != 1 || fread(&arg, 8, 1, f) != 1) break;
        if (head[0] == 0) {                                    /* tables: head[1] bit 0 dts, 1 pts, 2 flags, 3 plan only; arg = out_cap */
            hbs_mp4_stbl_write_params prm;
            if (fread(&prm, 32, 1, f) != 1) return 4;
            uint64_t* col[4] = {nullptr, nullptr, nullptr, nullptr};
            const bool have[4] = {true, true, (head[1] & 1) != 0, (head[1] & 2) != 0};
            for (int i = 0; i < 4; ++i) {
                if (!have[i]) continue;
                col[i] = (uint64_t*)malloc(n ? n * 8 : 1);     /* heap blocks of exactly N entries */
                if (n && fread(col[i], 8, n, f) != n) return 4;
            }
            uint32_t* fl = nullptr;
            if (head[1] & 4) { fl = (uint32_t*)malloc(n ? n * 4 : 1); if (n && fread(fl, 4, n, f) != n) return 4; }
            hbs::StblwIn in{col[0], col[1], n, col[2], col[3], fl, prm.sample_duration, prm.base_time, prm.data_offset};
            if (!hbs::mp4_stbl_write_params_ok(&prm)) printf("refused\n");
            else write(in, prm, (head[1] & 8) != 0, arg);
            for (int i = 0; i < 4; ++i) free(col[i]);
            free(fl);
        } else {                                               /* the moov: head[1] = flags, n = NALs, arg = duration; then tables_bytes */
            uint64_t tables_bytes;
            hbs_mp4_init_params p;
            if (fread(&tables_bytes, 8, 1, f) != 1 || fread(&p, 32, 1, f) != 1) return 4;
            std::vector<std::vector<uint8_t>> nals(n);
            for (auto& x : nals) {
                uint64_t k;
                if (fread(&k, 8, 1, f) != 1) return 4;
                x.resize(k);
                if (k && fread(x.data(), 1, k, f) != k) return 4;
            }
            moov(p, (int)head[1], nals, arg, tables_bytes);
        }
    }
    fclose(f);
    return 0;
}
"""


def digest(values):
    h = 0
    for v in values:
        h = (h * 1099511628211 + int(v)) & ((1 << 64) - 1)
    return h


def want_tables(c, plan, out_cap):
    p = c["params"]
    if p.get("reserved0") or p.get("base_time", 0) >> 62 or p.get("data_offset", 0) >> 62:
        return "refused"
    blob, rec, s = Wr.call({"t": c["t"], "params": {k: v for k, v in p.items() if k != "reserved0"}}, out_cap=None if plan else out_cap)
    tail = "%d %d %d %d %d" % (s["nal_count"], s["nal_found"], s["rbsp_bytes"], s["stream_bytes"], s["reserved"][1])
    if s["error"] == Wr.E_CAPACITY:
        return "capacity " + tail
    if s["error"]:
        return "sample %d" % (s["reserved"][2] - 1)
    if plan:
        return "plan " + tail
    words = np.frombuffer(blob, dtype=">u4").tolist()
    for name in Wr.ORDER:
        words += [int(rec[name][0][0]), int(rec[name][0][1])]
    return "ok %s %d" % (tail, digest(words))


def table_cases():
    """[(case, plan only, out_cap)]"""
    out = []
    rng = np.random.default_rng(91)
    for seed in range(12):
        n = int(rng.integers(0, 90)) if seed else 0
        t, _, dur = Wr.random_tables(rng, n, reorder=seed % 3 != 0, constant=5 if seed == 4 else None)
        if seed % 4 == 1:
            t["flags"] = None
        if seed % 5 == 2:
            t["dts"], t["pts"] = None, None
        c = Wr.case("random", t, sample_duration=dur, co64=bool(seed & 1), max_chunk_samples=(0, 0, 1, 3)[seed % 4], data_offset=seed * 1000, base_time=seed)
        T = Wr.call(c)[2]["stream_bytes"]
        out += [(c, True, 0), (c, False, T), (c, False, T - 1), (c, False, 0), (c, False, T + 100)]
    small = [c for c in Wr.valid_cases() if len(c["t"]["size"]) < 1000]
    out += [(c, False, 1 << 40) for c in small] + [(c, True, 0) for c in small[:6]]
    for c, _ in Wr.error_cases():
        out += [(c, False, 1 << 40), (c, True, 0)]
    c = small[2]
    for bad in (dict(reserved0=1), dict(base_time=1 << 62), dict(data_offset=1 << 62)):
        out.append((dict(c, params=dict(c["params"], **bad)), False, 1 << 40))
    return out


def moov_cases():
    """[(keyword arguments of moov_prefix)]"""
    out = [dict(duration=0, tables_bytes=0), dict(duration=123456, tables_bytes=4000, track_id=7, timescale=25, width=640, height=360, length_size=2),
           dict(duration=(1 << 32) - 1, tables_bytes=1 << 31, flags=1, bit_depth_luma=10, bit_depth_chroma=10, chroma_format_idc=2),
           dict(duration=1 << 32, tables_bytes=0), dict(duration=0, tables_bytes=2), dict(duration=0, tables_bytes=(1 << 32) - 4),
           dict(duration=0, tables_bytes=1 << 32), dict(duration=0, tables_bytes=0, track_id=0), dict(duration=0, tables_bytes=0, timescale=0),
           dict(duration=0, tables_bytes=0, width=0), dict(duration=0, tables_bytes=0, length_size=3), dict(duration=0, tables_bytes=0, flags=2)]
    prefix = Wr.moov_prefix(NALS, 0, 0)
    most = (Wr.M32 - (len(prefix) - int.from_bytes(prefix[:4], "big"))) // 4 * 4
    out += [dict(duration=5, tables_bytes=most), dict(duration=5, tables_bytes=most + 4)]
    return out


def test_rules_and_moov_under_sanitizers(tmp_path):
    from tests import _mp4_ref as R
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
    src = tmp_path / "mp4stblw_host_asan.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "mp4stblw_host_asan"
    cmd = [cxx] + flags + ["-I", os.path.join(ROOT, "hevcbitstream_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    tables, moovs = table_cases(), moov_cases()
    u64 = lambda x: np.array([v & ((1 << 64) - 1) for v in x], dtype=np.uint64).tobytes()          # noqa: E731
    with open(tmp_path / "cases.bin", "wb") as f:
        for c, plan, cap in tables:
            t, p = c["t"], c["params"]
            bits = (1 if t["dts"] is not None else 0) | (2 if t["pts"] is not None else 0) | (4 if t["flags"] is not None else 0) | (8 if plan else 0)
            prm = np.zeros(1, dtype=Wr.PARAMS)
            prm[0] = (Wr.CO64 if p.get("co64") else 0, p.get("max_chunk_samples", 0), p["sample_duration"], p.get("reserved0", 0), p.get("base_time", 0),
                      p.get("data_offset", 0))
            f.write(struct.pack("<IIQQ", 0, bits, len(t["size"]), cap) + prm.tobytes() + u64(t["off"]) + u64(t["size"]))
            for name in ("dts", "pts"):
                if t[name] is not None:
                    f.write(u64(t[name]))
            if t["flags"] is not None:
                f.write(np.array(t["flags"], dtype=np.uint32).tobytes())
        for kw in moovs:
            prm = np.zeros(1, dtype=R.INIT_PARAMS)
            prm[0] = (kw.get("track_id", 1), kw.get("timescale", 90000), kw.get("width", 1920), kw.get("height", 1080), kw.get("length_size", 4),
                      kw.get("chroma_format_idc", 1), kw.get("bit_depth_luma", 8), kw.get("bit_depth_chroma", 8))
            f.write(struct.pack("<IIQQQ", 1, kw.get("flags", 0), len(NALS), kw["duration"], kw["tables_bytes"]) + prm.tobytes())
            for x in NALS:
                f.write(struct.pack("<Q", len(x)) + bytes(x))
    run = subprocess.run([str(exe), str(tmp_path / "cases.bin")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-6000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(tables) + len(moovs)
    verdicts = set()
    for i, ((c, plan, cap), got) in enumerate(zip(tables, lines)):
        assert got == want_tables(c, plan, cap), (i, c["name"], plan, cap)
        verdicts.add("tables " + got.split()[0])
    for kw, got in zip(moovs, lines[len(tables):]):
        want = Wr.moov_prefix(NALS, **kw)
        assert got == ("refused" if want == Wr.E_ARG else "moov %d %d" % (len(want), digest(want))), kw
        verdicts.add(got.split()[0])
    assert verdicts == {"tables ok", "tables plan", "tables capacity", "tables sample", "tables refused", "moov", "refused"}
