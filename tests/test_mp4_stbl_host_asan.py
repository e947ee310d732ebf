"""The host/device rules of hbs_mp4stbl.h (stbl_heads, stbl_stsc_entry, stbl_stss_entry, stbl_run_samples, stbl_join, stbl_place)
, hbs_mp4_stbl_find_host and hbs_mp4_track_read_host under AddressSanitizer and UBSan, in a stand-alone program: a plain host loop over the rule
functions -- the six fixed parts, every entry, every sample -- on tables in exactly sized heap blocks: valid ones, ones with
every kind of error, counts of 2^32 - 1, every payload cut short at every length; and the finder and the track reader on whole files, on a moov cut
at every length and on a moov with single bytes of its size, type and version fields altered.  The program prints what it
accepted and a digest of every table; the reader and the finder of tests/_mp4_stbl_ref.py must say the same of every block.
Nothing is loaded into python."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import _mp4_stbl_ref as S
from tests._mp4_read_ref import Malformed, boxes
from tests.test_mp4_read_ref import NALS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "hevcbitstream_amd.h"
#include "hbs_mp4stbl.h"

static uint64_t h;
static void mix(uint64_t v) { h = h * 1099511628211ull + v; }

/* hbs_mp4_stbl_samples on the host: one loop over the entries, one over the samples */
static void tables(const uint8_t* p, uint64_t n, const hbs_mp4_stbl& t, bool outputs, uint64_t cap)
{
    using namespace hbs;
    const hbs_mp4_box_ref* ref[kStBoxes] = {&t.stsz, &t.stco, &t.stsc, &t.stts, &t.ctts, &t.stss};
    StblBox box[kStBoxes];
    for (int b = 0; b < kStBoxes; ++b) { box[b].off = ref[b]->off; box[b].bytes = ref[b]->bytes; }
    const bool co64 = (t.flags & HBS_MP4_STBL_CO64) != 0;
    const uint64_t file_bytes = t.file_bytes ? t.file_bytes : n;
    StblHead hd;
    stbl_heads(p, box, co64, hd);
    uint64_t bad = hd.bad;
    auto worse = [&](uint64_t b) { if (!bad || b < bad) bad = b; };
    std::vector<uint64_t> sfirst(hd.E), tfirst(hd.T), ttime(hd.T), cfirst(hd.K);
    uint64_t s0 = 0, t0 = 0, hi = 0, lo = 0, c0 = 0;
    for (uint64_t e = 0; e < hd.E; ++e) {
        uint32_t fc, spc;
        uint64_t chunks;
        sfirst[e] = s0;
        if (stbl_stsc_entry(p, box[kStsc].off + 8, e, hd.E, hd.C, fc, spc, chunks)) s0 += stbl_run_samples(chunks, spc);
        else worse(1 + kStsc);
    }
    if (s0 < hd.N) worse(1 + kStsc);
    for (uint64_t i = 0; i < hd.T; ++i) {
        const uint64_t cnt = rd_be32(p, box[kStts].off + 8 + i * 8), prod = cnt * rd_be32(p, box[kStts].off + 12 + i * 8);
        tfirst[i] = t0; ttime[i] = stbl_join(hi, lo);
        t0 += cnt; hi += prod >> 32; lo += prod & 0xFFFFFFFFull;
    }
    if (t0 < hd.N) worse(1 + kStts);
    for (uint64_t i = 0; i < hd.K; ++i) { cfirst[i] = c0; c0 += rd_be32(p, box[kCtts].off + 8 + i * 8); }
    for (uint64_t i = 0; i < hd.S; ++i) {
        uint32_t number;
        if (!stbl_stss_entry(p, box[kStss].off + 8, i, number)) worse(1 + kStss);
    }
    if (bad) { printf("table %llu\n", (unsigned long long)bad); return; }
    if (!outputs) {
        uint64_t bytes = hd.N * hd.ssz;
        if (!hd.ssz) for (uint64_t k = 0; k < hd.N; ++k) bytes += rd_be32(p, box[kStsz].off + 12 + k * 4);
        printf("plan %llu %llu %llu\n", (unsigned long long)hd.N, (unsigned long long)hd.C, (unsigned long long)bytes);
        return;
    }
    if (hd.N > cap) { printf("capacity %llu %llu\n", (unsigned long long)hd.N, (unsigned long long)hd.C); return; }
    h = 0;
    uint64_t e = 0, ti = 0, ci = 0, si = 0, before = 0, bytes = 0;
    for (uint64_t k = 0; k < hd.N; ++k) {
        while (e + 1 < hd.E && sfirst[e + 1] <= k) ++e;
        while (ti + 1 < hd.T && tfirst[ti + 1] <= k) ++ti;
        while (ci + 1 < hd.K && cfirst[ci + 1] <= k) ++ci;
        const uint32_t size = hd.ssz ? hd.ssz : rd_be32(p, box[kStsz].off + 12 + k * 4);
        const uint32_t fc = rd_be32(p, box[kStsc].off + 8 + e * 12), spc = rd_be32(p, box[kStsc].off + 12 + e * 12);
        const uint32_t r = (uint32_t)(k - sfirst[e]);
        const uint64_t chunk = (uint64_t)(fc - 1) + r / spc;
        if (r % spc == 0) before = 0;
        const uint64_t chunk_off = co64 ? rd_be64(p, box[kStco].off + 8 + chunk * 8) : rd_be32(p, box[kStco].off + 8 + chunk * 4);
        int64_t cts = 0;
        if (hd.K && k - cfirst[ci] < rd_be32(p, box[kCtts].off + 8 + ci * 8)) cts = stbl_cts(rd_be32(p, box[kCtts].off + 12 + ci * 8), hd.ctts_v);
        uint64_t off, dts, pts;
        if (!stbl_place(chunk_off, before, size, file_bytes, ttime[ti], k - tfirst[ti], rd_be32(p, box[kStts].off + 12 + ti * 8), cts, off, dts, pts)) {
            printf("sample %llu\n", (unsigned long long)k);
            return;
        }
        bool sync = box[kStss].bytes == 0;
        if (!sync) {
            while (si < hd.S && rd_be32(p, box[kStss].off + 8 + si * 4) < k + 1) ++si;
            sync = si < hd.S && rd_be32(p, box[kStss].off + 8 + si * 4) == k + 1;
        }
        mix(off); mix(size); mix(dts); mix(pts); mix(sync ? 0 : 0x00010000);
        before += size; bytes += size;
    }
    printf("ok %llu %llu %llu %llu\n", (unsigned long long)hd.N, (unsigned long long)hd.C, (unsigned long long)bytes, (unsigned long long)h);
}

static void find(const uint8_t* p, uint64_t n, uint64_t base, uint32_t track)
{
    hbs_mp4_stbl t;
    if (hbs::mp4_stbl_find_host(p, n, base, track, &t) != 0) { printf("refused\n"); return; }
    h = 0;
    const uint64_t* w = reinterpret_cast<const uint64_t*>(&t);
    for (int i = 0; i < 16; ++i) mix(w[i]);
    printf("found %llu\n", (unsigned long long)h);
}

static void track(const uint8_t* p, uint64_t n, uint32_t id)
{
    hbs_mp4_track t;
    uint64_t off[64], size[64];
    const int64_t got = hbs::mp4_track_read_host(p, n, id, &t, off, size, 64);
    if (got < 0) { printf("refused\n"); return; }
    h = 0;
    mix(t.track_id); mix(t.timescale); mix(t.width); mix(t.height); mix((uint64_t)t.length_size); mix(t.entry);
    mix(t.trex_duration); mix(t.trex_size); mix(t.trex_flags); mix(t.n_nals); mix(t.hvcc_off); mix(t.hvcc_bytes);
    for (int64_t i = 0; i < got && i < 64; ++i) { mix(off[i]); mix(size[i]); }
    printf("track %lld %llu\n", (long long)got, (unsigned long long)h);
}

/* the limits no table of a testable size reaches: 2^62 in the times, 2^32 samples in a run */
static int limits()
{
    using namespace hbs;
    const uint64_t L = 1ull << 62, M = 0xFFFFFFFFull;
    uint64_t off, dts, pts;
    int bad = 0;
    bad |= stbl_join(0, 0) != 0 || stbl_join(1, 5) != (1ull << 32) + 5 || stbl_join((1ull << 30) - 1, M) != L - 1;
    bad |= stbl_join(1ull << 30, 0) != L || stbl_join((1ull << 30) - 1, 1ull << 32) != L || stbl_join(0, L) != L || stbl_join(~0ull, ~0ull) != L;
    bad |= stbl_join((1ull << 30) - 1, M + 1) != L || stbl_join(0, L - 1) != L - 1 || stbl_join(M * M >> 32, 0) != L;
    bad |= stbl_run_samples(M, (uint32_t)M) != (1ull << 32) || stbl_run_samples(1ull << 16, 1u << 16) != (1ull << 32) || stbl_run_samples(65535, 65537) != M;
    bad |= stbl_run_samples(0, (uint32_t)M) != 0 || stbl_run_samples(M, 0) != 0;
    bad |= !stbl_place(0, 0, 0, 0, L - 1, 0, 0, 0, off, dts, pts) || dts != L - 1 || pts != L - 1;
    bad |= stbl_place(0, 0, 0, 0, L, 0, 0, 0, off, dts, pts) || stbl_place(0, 0, 0, 0, L - 1, 1, 1, 0, off, dts, pts);
    bad |= stbl_place(0, 0, 0, 0, 0, M, (uint32_t)M, 0, off, dts, pts) || !stbl_place(0, 0, 0, 0, 0, 1ull << 30, (uint32_t)M, 0, off, dts, pts);
    bad |= stbl_place(0, 0, 0, 0, L - 1, 0, 0, 1, off, dts, pts) || stbl_place(0, 0, 0, 0, 4, 0, 0, -5, off, dts, pts);
    bad |= !stbl_place(0, 0, 0, 0, 4, 1, 1, -5, off, dts, pts) || pts != 0 || dts != 5;
    bad |= stbl_place(~0ull, 0, 0, L, 0, 0, 0, 0, off, dts, pts) || stbl_place(L, 1, 0, L, 0, 0, 0, 0, off, dts, pts);
    bad |= stbl_place(L - 1, ~0ull, 1, L, 0, 0, 0, 0, off, dts, pts) || stbl_place(L - 4, 2, 3, L, 0, 0, 0, 0, off, dts, pts);
    bad |= !stbl_place(L - 4, 2, 2, L, 0, 0, 0, 0, off, dts, pts) || off != L - 2;
    return bad;
}

int main(int argc, char** argv)
{
    static_assert(sizeof(hbs_mp4_stbl) == 128, "hbs_mp4_stbl");
    if (limits()) return 5;
    FILE* f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    if (!f) return 3;
    for (;;) {
        uint32_t head[2];
        uint64_t arg, n;
        hbs_mp4_stbl t;
        if (fread(head, 4, 2, f) != 2 || fread(&arg, 8, 1, f) != 1 || fread(&n, 8, 1, f) != 1 || fread(&t, 128, 1, f) != 1) break;
        uint8_t* p = (uint8_t*)malloc(n ? n : 1);              /* a heap block of exactly n bytes */
        if (n && fread(p, 1, n, f) != n) return 4;
        if (head[0] == 0) tables(p, n, t, head[1] != 0, arg);
        else if (head[0] == 1) find(p, n, arg, head[1]);
        else track(p, n, head[1]);
        free(p);
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


def want_tables(buf, rec, outputs, cap):
    off, size, dts, pts, fl, s = S.read(buf, rec, sample_cap=cap, outputs=outputs)
    if s["error"] == S.E_CAPACITY:
        return "capacity %d %d" % (s["nal_count"], s["nal_found"])
    if s["error"]:
        return "table %d" % s["reserved"][0] if s["reserved"][0] else "sample %d" % (s["reserved"][2] - 1)
    if not outputs:
        return "plan %d %d %d" % (s["nal_count"], s["nal_found"], s["rbsp_bytes"])
    vals = []
    for k in range(len(off)):
        vals += [off[k], size[k], dts[k], pts[k], fl[k]]
    return "ok %d %d %d %d" % (s["nal_count"], s["nal_found"], s["rbsp_bytes"], digest(vals))


def want_find(buf, base, track):
    try:
        rec = S.find(buf, base, track)
    except Malformed:
        return "refused"
    return "found %d" % digest(np.frombuffer(rec.tobytes(), dtype="<u8"))


def want_track(buf, track):
    try:
        t, nals = S.track_read(buf, track)
    except Malformed:
        return "refused"
    vals = [t[k] for k in ("track_id", "timescale", "width", "height", "length_size", "entry", "trex_duration", "trex_size", "trex_flags",
                           "n_nals", "hvcc_off", "hvcc_bytes")]
    for o, n in nals:
        vals += [o, n]
    return "track %d %d" % (len(nals), digest(vals))


def field_bytes(buf):
    """the offsets of every size, type and version byte, and of the counts, of every box the finder walks into"""
    at = set()

    def go(lo, hi, depth):
        try:
            found = boxes(buf, lo, hi)
        except Malformed:
            return
        for kind, s, p, e in found:
            at.update(range(s, min(p + 8, e)))
            if kind in (b"moov", b"trak", b"mdia", b"minf", b"stbl") and depth < 8:
                go(p, e, depth + 1)
    go(0, len(buf), 0)
    return sorted(at)


def table_cases():
    """[(buffer, record, outputs, sample_cap)]"""
    out = []
    rng = np.random.default_rng(77)
    M = S.M32
    for seed in range(10):
        n = int(rng.integers(0, 90))
        t = S.random_track(rng, n, reorder=seed % 3 != 0, constant=5 if seed == 4 else None)
        offs, at = [], 0
        for c in t["chunk_lens"]:
            offs.append(at)
            at += 500
        co64 = bool(seed & 1)
        if co64:
            offs = [o + (1 << 33) for o in offs]
        pay = S.payloads([len(x) for x in t["samples"]], t["chunk_lens"], offs, t["deltas"], t["cts"], None if seed == 2 else t["sync"], co64,
                         5 if seed == 4 else None)
        buf, rec = S.layout(pay, lead=seed, align=seed)
        rec["flags"] = S.CO64 if co64 else 0
        rec["file_bytes"] = 1 << 40
        out += [(buf, rec, True, n), (buf, rec, False, 0), (buf, rec, True, max(n - 1, 0))]
        # a file that ends inside some sample, and every payload cut short at every length, the box last in an exact block
        small = rec.copy()
        small["file_bytes"] = (offs[len(offs) // 2] + 3) if offs else 1
        out.append((buf, small, True, n))
        if seed < 4:
            for name in S.BOXES:
                if pay[name] is None:
                    continue
                order = [x for x in S.BOXES if x != name] + [name]
                for cut in range(0 if name in ("ctts", "stss") else 1, len(pay[name])):
                    p2 = dict(pay)
                    p2[name] = pay[name][:cut] or None
                    b2, r2 = S.layout(p2, order=order)
                    r2["flags"], r2["file_bytes"] = rec["flags"], rec["file_bytes"]
                    out.append((b2, r2, True, n))
    # every table error and sample error on a small track
    sizes, lens, offs, deltas = [4, 5, 6, 7], [3, 1], [100, 200], [10, 10, 10, 10]
    base = S.payloads(sizes, lens, offs, deltas, cts=[0, 5, 0, 0], sync=[0, 2])
    changes = [{}, {"stsz": S.p_stsz(sizes, count=5)}, {"stsz": S.p_stsz(sizes, version=1)}, {"stco": S.p_stco(offs, version=1)},
               {"stco": S.p_stco(offs, count=3)}, {"stsc": S.p_stsc([(1, 3), (1, 1)])}, {"stsc": S.p_stsc([(1, 3), (3, 1)])},
               {"stsc": S.p_stsc([(2, 3)])}, {"stsc": S.p_stsc([(1, 1)])}, {"stsc": S.p_stsc([(1, 0), (2, 4)])}, {"stsc": S.p_stsc([(1, 3), (2, 0)])},
               {"stsc": S.p_stsc([(1, 3)], version=1)}, {"stsc": S.p_stsc([])}, {"stts": S.p_pairs([(3, 10)])}, {"stts": S.p_pairs([(0, 7), (9, 1), (0, 3)])},
               {"stts": S.p_pairs([(4, 1)], version=1)}, {"ctts": S.p_pairs([(1, 0)], version=2)}, {"ctts": S.p_pairs([(1, 7)], count=2)},
               {"ctts": S.p_pairs([(0, 9), (2, M)])}, {"ctts": S.p_pairs([(2, 0), (1, -21)], version=1, signed=True)},
               {"ctts": S.p_pairs([(2, 0), (1, -20)], version=1, signed=True)}, {"stss": S.p_stss([2, 2])}, {"stss": S.p_stss([0])},
               {"stss": S.p_stss([1, 9])}, {"stss": S.p_stss([])}, {"stss": S.p_stss([3], version=1)}, {"stts": S.p_pairs([(3, 10)]), "stss": S.p_stss([0])},
               {"stts": S.p_pairs([(2, 1 << 31), (2, M)]), "ctts": None}, {"stts": S.p_pairs([(1, M)] * 3 + [(1, 0)]), "ctts": None},
               {"stco": S.p_stco([100, (1 << 32) - 3])}]
    for ch in changes:
        p = dict(base)
        p.update(ch)
        buf, rec = S.layout(p, lead=3)
        for fb in (1000, 114, 1 << 40):
            rec = rec.copy()
            rec["file_bytes"] = fb
            out += [(buf, rec, True, 4), (buf, rec, False, 0)]
    # counts of 2^32 - 1, whose sums and products pass 2^64: plan only -- and with outputs a capacity error
    huge = dict(stsz=S.p_stsz([], constant=7, count=M), stco=S.p_stco([0] * 3), stsc=S.p_stsc([(1, M)]), stts=S.p_pairs([(M, M)]), ctts=None, stss=None)
    for ch in ({}, {"stsc": S.p_stsc([(1, 1), (2, M)])}, {"stsc": S.p_stsc([(1, 1)])}, {"stts": S.p_pairs([(M - 1, 1)])}, {"stts": S.p_pairs([(M, M)] * 5)},
               {"stsz": S.p_stsz([], constant=0, count=M)}, {"stsc": S.p_stsc([(1, M), (2, M), (3, M)])}):
        p = dict(huge)
        p.update(ch)
        buf, rec = S.layout(p)
        rec["file_bytes"] = 1 << 62
        out += [(buf, rec, False, 0), (buf, rec, True, 100)]
    # 64 samples with the largest deltas there are (2^62 takes 2^30 of them: the program checks that limit on the rules alone)
    p = S.payloads([1] * 64, [64], [0], [0] * 64)
    p["stts"] = S.p_pairs([(1, M)] * 40 + [(24, M)])
    buf, rec = S.layout(p)
    rec["file_bytes"] = 1000
    out.append((buf, rec, True, 64))
    return out


def find_cases():
    """[(buffer, base, track_id)]"""
    out = []
    rng = np.random.default_rng(5)
    for seed in range(3):
        t = S.random_track(rng, 20 + seed)
        data, _ = S.progressive_file(t["samples"], t["chunk_lens"], t["deltas"], t["cts"], t["sync"] if seed else None, nals=NALS, track_id=7,
                                     co64=seed == 1, moov_first=seed != 2)
        data = bytes(data)
        out += [(data, 0, 0), (data, 0, 7), (data, 0, 8), (data, 12345, 0)]
        at = data.index(b"moov") - 4
        moov = data[at:at + int.from_bytes(data[at:at + 4], "big")]
        out += [(moov, at, 0)]
        out += [(moov[:n], at, 0) for n in range(len(moov))]
        for pos in field_bytes(moov):
            for v in (0, 1, moov[pos] ^ 1, 0xFF):
                if v != moov[pos]:
                    out.append((moov[:pos] + bytes([v]) + moov[pos + 1:], 0, 0))
        # a moov whose last box runs to its end (size 0), and one without each table box in turn
        for kind in (b"stsz", b"stco", b"co64", b"stsc", b"stts", b"ctts", b"stss"):
            if kind in moov:
                pos = moov.index(kind)
                out.append((moov[:pos] + b"free" + moov[pos + 4:], 0, 0))
                out.append((moov[:pos] + b"stz2" + moov[pos + 4:], 0, 0))
    return out


def test_rules_and_finder_under_sanitizers(tmp_path):
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
    src = tmp_path / "mp4stbl_host_asan.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "mp4stbl_host_asan"
    cmd = [cxx] + flags + ["-I", os.path.join(ROOT, "hevcbitstream_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    tables, finds = table_cases(), find_cases()
    with open(tmp_path / "cases.bin", "wb") as f:
        for buf, rec, outputs, cap in tables:
            f.write(struct.pack("<IIQQ", 0, int(outputs), cap, len(buf)) + rec.tobytes() + buf)
        for kind in (1, 2):                                # the finder, then the track reader on the same blocks
            for buf, base, track in finds:
                f.write(struct.pack("<IIQQ", kind, track, base, len(buf)) + bytes(128) + buf)
    run = subprocess.run([str(exe), str(tmp_path / "cases.bin")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-6000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(tables) + 2 * len(finds)
    verdicts = set()
    for i, ((buf, rec, outputs, cap), got) in enumerate(zip(tables, lines)):
        assert got == want_tables(buf, rec, outputs, cap), (i, outputs, cap, rec)
        verdicts.add(got.split()[0] + (" " + got.split()[1] if got.startswith("table") else ""))
    for i, ((buf, base, track), got) in enumerate(zip(finds, lines[len(tables):])):
        assert got == want_find(buf, base, track), (i, len(buf), base, track)
        verdicts.add(got.split()[0])
    for i, ((buf, base, track), got) in enumerate(zip(finds, lines[len(tables) + len(finds):])):
        assert got == want_track(buf, track), (i, len(buf), track)
        verdicts.add(got.split()[0])
    assert verdicts == {"ok", "plan", "capacity", "sample", "found", "track", "refused"} | {"table %d" % b for b in range(1, 7)}
