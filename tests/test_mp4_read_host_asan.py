"""The host/device rules of hbs_mp4rd.h (mp4rd_box, mp4rd_moof, mp4rd_sample, mp4rd_place) and the init segment's reader under
AddressSanitizer and UBSan, in a stand-alone program: a plain host loop over the rule functions -- the chain of top-level
boxes, every moof, every sample -- on segments and init segments in exactly sized heap blocks: valid ones, their truncations
at every length, and valid ones with single bytes of the size and flag fields altered; and a two-track init segment, clear
and protected, at every truncation through the reader, mp4_init_protect and mp4_init_unprotect (hbs_mp4prot.h,
hbs_mp4senc.h), which share the reader's walk.  The program prints what it accepted and a digest of every table and every
byte written; the box-by-box readers of tests/_mp4_read_ref.py, _mp4_protect_ref.py and _mp4_senc_ref.py must say the same
of every block.  Nothing is loaded into python."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import _mp4_protect_ref as P
from tests import _mp4_ref as R
from tests import _mp4_read_ref as Q
from tests import _mp4_senc_ref as S
from tests.test_mp4_init_mutations import PSSH, TENC, two_tracks
from tests.test_mp4_read_ref import NALS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "hbs_mp4senc.h"

static uint64_t h;
static void mix(uint64_t v) { h = h * 1099511628211ull + v; }

struct MoofAt { uint64_t at, size; uint32_t head; };

/* one segment, the block: the loop of hbs_mp4_samples on the host */
static void samples(const uint8_t* p, uint64_t n, const hbs::Mp4Trex& x)
{
    std::vector<MoofAt> moofs;
    for (uint64_t q = 0; q < n;) {
        hbs::Mp4Box b;
        if (!hbs::mp4rd_box(p, q, n, b)) { printf("chain\n"); return; }
        if (b.type == HBS_MP4_FOURCC('m', 'o', 'o', 'f')) moofs.push_back({q, b.size, b.head});
        q += b.size;
    }
    /* what the plan-only kernel does: a step an entry that has bytes, the closed form for a trun whose entries have none */
    uint64_t k = 0, bytes = 0, bad_sample = 0;
    std::vector<std::vector<hbs::Mp4TrunRec>> all(moofs.size());
    std::vector<hbs::Mp4Moof> info(moofs.size());
    for (size_t m = 0; m < moofs.size(); ++m) {
        std::vector<hbs::Mp4TrunRec>& recs = all[m];
        if (!hbs::mp4rd_moof(p, 0, moofs[m].at, moofs[m].size, moofs[m].head, x, info[m], [&](uint64_t, const hbs::Mp4TrunRec& r) { recs.push_back(r); })) {
            printf("moof %zu\n", m);
            return;
        }
        uint64_t before = 0, dur_before = 0;
        for (size_t i = 0; i < recs.size() && !bad_sample; ++i) {
            const hbs::Mp4TrunRec& r = recs[i];
            if (r.tr & hbs::kRdHead) before = 0;
            if (hbs::mp4rd_entry_bytes(r.tr) == 0) {
                const uint64_t good = hbs::mp4rd_run_good(r.begin, before, r.def_size, n, r.tfdt, dur_before, r.def_dur, r.count);
                if (good < r.count) { bad_sample = k + good + 1; break; }
                before += (uint64_t)r.count * r.def_size; bytes += (uint64_t)r.count * r.def_size; dur_before += (uint64_t)r.count * r.def_dur;
                k += r.count;
                continue;
            }
            for (uint32_t e = 0; e < r.count; ++e, ++k) {
                const hbs::Mp4Sample s = hbs::mp4rd_sample(p, r, e);
                uint64_t off, dts, pts;
                if (!hbs::mp4rd_place(r.begin, before, s.size, n, r.tfdt, dur_before, s.cts, off, dts, pts)) { bad_sample = k + 1; break; }
                before += s.size; dur_before += s.dur; bytes += s.size;
            }
        }
        if (bad_sample) break;
    }
    if (bad_sample) { printf("sample %llu\n", (unsigned long long)(bad_sample - 1)); return; }
    if (k > 65536) { printf("big %llu %zu %llu\n", (unsigned long long)k, moofs.size(), (unsigned long long)bytes); return; }
    /* few enough to list: every sample one by one, as the sample kernels see them; the closed form must have said the same */
    h = 0; k = 0;
    for (size_t m = 0; m < moofs.size(); ++m) {
        uint64_t before = 0, dur_before = 0;
        uint32_t first_flags = 0x00010000u;
        const uint64_t k0 = k;
        for (size_t i = 0; i < all[m].size(); ++i) {
            const hbs::Mp4TrunRec& r = all[m][i];
            if (r.tr & hbs::kRdHead) before = 0;
            for (uint32_t e = 0; e < r.count; ++e, ++k) {
                const hbs::Mp4Sample s = hbs::mp4rd_sample(p, r, e);
                if (k == k0) first_flags = s.flags;
                uint64_t off, dts, pts;
                if (!hbs::mp4rd_place(r.begin, before, s.size, n, r.tfdt, dur_before, s.cts, off, dts, pts)) { printf("closed form and loop disagree at %llu\n", (unsigned long long)k); return; }
                mix(off); mix(s.size); mix(dts); mix(pts); mix(s.flags);
                before += s.size; dur_before += s.dur;
            }
        }
        mix(moofs[m].at); mix(k0); mix(info[m].tfdt); mix(info[m].samples); mix(info[m].sequence);
        mix((info[m].samples && hbs::mp4rd_sync(first_flags)) ? 1 : 0);
    }
    printf("ok %llu %zu %llu %llu\n", (unsigned long long)k, moofs.size(), (unsigned long long)bytes, (unsigned long long)h);
}

static void init(const uint8_t* p, uint64_t n, uint32_t track)
{
    hbs_mp4_track t;
    uint64_t off[64], size[64];
    const int64_t got = hbs::mp4_init_read_host(p, n, track, &t, off, size, 64);
    if (got < 0) { printf("refused\n"); return; }
    h = 0;
    mix(t.track_id); mix(t.timescale); mix(t.width); mix(t.height); mix((uint64_t)t.length_size); mix(t.entry);
    mix(t.trex_duration); mix(t.trex_size); mix(t.trex_flags); mix(t.n_nals); mix(t.hvcc_off); mix(t.hvcc_bytes);
    for (int64_t i = 0; i < got && i < 64; ++i) { mix(off[i]); mix(size[i]); }
    printf("ok %lld %llu\n", (long long)got, (unsigned long long)h);
}

static const uint8_t kTenc[64] = {@TENC@};
static const uint8_t kPssh[] = {@PSSH@};

/* the two rewriters: the size first, then into a heap block of exactly that size */
static void protect(const uint8_t* p, uint64_t n, uint32_t track)
{
    hbs_mp4_tenc t;
    memcpy(&t, kTenc, sizeof(t));
    const uint8_t* boxes[1] = {kPssh};
    const uint64_t sizes[1] = {sizeof(kPssh)};
    const int64_t need = hbs::mp4_init_protect(p, n, track, &t, boxes, sizes, 1, nullptr, 0);
    if (need < 0) { printf("refused\n"); return; }
    uint8_t* out = (uint8_t*)malloc((size_t)need);
    if (hbs::mp4_init_protect(p, n, track, &t, boxes, sizes, 1, out, (uint64_t)need) != need) { printf("the second call disagrees\n"); free(out); return; }
    h = 0;
    for (int64_t i = 0; i < need; ++i) mix(out[i]);
    free(out);
    printf("ok %lld %llu\n", (long long)need, (unsigned long long)h);
}

static void unprotect(const uint8_t* p, uint64_t n, uint32_t track)
{
    hbs_mp4_tenc t;
    uint32_t format = 0;
    uint64_t n_pssh = 0;
    const int64_t need = hbs::mp4_init_unprotect(p, n, track, &t, &format, nullptr, nullptr, 0, &n_pssh, nullptr, 0);
    if (need < 0) { printf("refused\n"); return; }
    uint8_t* out = (uint8_t*)malloc((size_t)need);
    uint64_t* off = (uint64_t*)malloc(n_pssh ? n_pssh * 8 : 1);
    uint64_t* size = (uint64_t*)malloc(n_pssh ? n_pssh * 8 : 1);
    const int64_t got = hbs::mp4_init_unprotect(p, n, track, &t, &format, off, size, n_pssh, &n_pssh, out, (uint64_t)need);
    h = 0;
    mix(format); mix(n_pssh);
    for (uint64_t i = 0; i < n_pssh; ++i) { mix(off[i]); mix(size[i]); }
    for (size_t i = 0; i < sizeof(t); ++i) mix(((const uint8_t*)&t)[i]);
    for (int64_t i = 0; i < need; ++i) mix(out[i]);
    free(out); free(off); free(size);
    if (got != need) printf("the second call disagrees\n");
    else printf("ok %lld %llu\n", (long long)need, (unsigned long long)h);
}

int main(int argc, char** argv)
{
    FILE* f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    if (!f) return 3;
    for (;;) {
        uint32_t head[5];
        uint64_t n;
        if (fread(head, 4, 5, f) != 5 || fread(&n, 8, 1, f) != 1) break;
        uint8_t* p = (uint8_t*)malloc(n ? n : 1);              /* a heap block of exactly n bytes */
        if (n && fread(p, 1, n, f) != n) return 4;
        if (!n) { free(p); p = nullptr; }
        if (head[0] == 0) {
            hbs::Mp4Trex x;
            x.track_id = head[1]; x.dur = head[2]; x.size = head[3]; x.flags = head[4];
            if (p || !n) samples(p, n, x);
        } else if (head[0] == 1) init(p, n, head[1]);
        else if (head[0] == 2) protect(p, n, head[1]);
        else unprotect(p, n, head[1]);
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


def want_samples(buf, prm):
    s = Q.samples(buf, None, prm, tables=False)[6]
    if s["error"]:
        r = s["reserved"]
        return "chain" if r[0] else "moof %d" % (r[1] - 1) if r[1] else "sample %d" % (r[2] - 1)
    if s["nal_count"] > 65536:
        return "big %d %d %d" % (s["nal_count"], s["nal_found"], s["rbsp_bytes"])
    off, size, dts, pts, fl, frags, s = Q.samples(buf, None, prm)
    vals, k = [], 0
    for f in frags:
        for _ in range(int(f["samples"])):
            vals += [off[k], size[k], dts[k], pts[k], fl[k]]
            k += 1
        vals += [f["out_off"], f["first_au"], f["decode_time"], f["samples"], f["sequence"], f["flags"]]
    return "ok %d %d %d %d" % (s["nal_count"], s["nal_found"], s["rbsp_bytes"], digest(vals))


def want_init(buf, track):
    try:
        t, nals = Q.init_read(buf, track)
    except Q.Malformed:
        return "refused"
    vals = [t[k] for k in ("track_id", "timescale", "width", "height", "length_size", "entry", "trex_duration", "trex_size", "trex_flags",
                           "n_nals", "hvcc_off", "hvcc_bytes")]
    for o, n in nals:
        vals += [o, n]
    return "ok %d %d" % (len(nals), digest(vals))


def want_protect(buf, track):
    out = P.init_protect(buf, TENC, PSSH, track)
    return "refused" if out == P.E_ARG else "ok %d %d" % (len(out), digest(out))


def want_unprotect(buf, track):
    got = S.init_unprotect(buf, track)
    if got == S.E_ARG:
        return "refused"
    out, tenc, fmt, pssh = got
    return "ok %d %d" % (len(out), digest([fmt, len(pssh)] + [v for pair in pssh for v in pair] + list(tenc.tobytes()) + list(out)))


def field_bytes(buf):
    """the offsets of every size, type, version and flag byte, and of the counts, of every box the reader walks into"""
    at = set()

    def go(lo, hi, depth):
        try:
            found = Q.boxes(buf, lo, hi)
        except Q.Malformed:
            return
        for kind, s, p, e in found:
            at.update(range(s, min(p + 8, e)))
            if kind in (b"moof", b"traf", b"moov", b"trak", b"mdia", b"minf", b"stbl", b"mvex") and depth < 8:
                go(p, e, depth + 1)
    go(0, len(buf), 0)
    return sorted(at)


def cases():
    out = []
    rng = np.random.default_rng(2024)
    for seed in range(6):
        prm = Q.read_params(track_id=seed % 3, trex_duration=100 + seed, trex_size=seed, trex_flags=0x01010000 * (seed & 1))
        buf, segs, _, _ = Q.random_segments(rng, 1, prm, moofs_per_seg=(1, 2))
        out.append((0, prm, buf))
        step = 1 if seed < 2 else 7
        out += [(0, prm, buf[:n]) for n in range(0, len(buf), step)]
        for at in field_bytes(buf)[:: 1 if seed < 2 else 3]:
            for v in (0, 1, buf[at] ^ 1, buf[at] ^ 0x80, 0xFF):
                if v != buf[at]:
                    out.append((0, prm, buf[:at] + bytes([v]) + buf[at + 1:]))
    # truns whose entries have no bytes: the count is bounded by nothing in the box
    prm = Q.read_params(track_id=1, trex_duration=0, trex_size=0)
    for count in (1, 4097, 70000, (1 << 24) + 5, (1 << 32) - 1):
        for hflags, dur, size in ((0x020000, 0, 0), (0x020008, 1 << 31, 0), (0x020010, 0, 1), (0x020018, 3, 2), (0x020018, (1 << 32) - 1, 0)):
            for tflags, off in ((0, 0), (5, 40), (1, -1)):
                traf = Q.tfhd(1, hflags, dur=dur, size=size) + Q.tfdt(77) + Q.trun(0x200, [(0, 3, 0, 0)]) + Q.trun(tflags, [], 0, off, 0x02000000, count=count)
                out.append((0, prm, Q.box(b"moof", Q.mfhd(1) + Q.box(b"traf", traf + Q.trun(0x100, [(9, 0, 0, 0)]))) + Q.box(b"mdat", bytes(300))))
    for L, flags in ((4, 0), (1, R.HEV1)):
        seg = bytes(R.init_segment(NALS, track_id=7, timescale=24000, width=1280, height=720, length_size=L, flags=flags))
        for track in (0, 7, 8):
            out.append((1, dict(track_id=track), seg))
        out += [(1, dict(track_id=0), seg[:n]) for n in range(len(seg))]
        for at in field_bytes(seg) + list(range(len(seg) - 150, len(seg))):
            for v in (0, 1, seg[at] ^ 1, 0xFF):
                if v != seg[at]:
                    out.append((1, dict(track_id=0), seg[:at] + bytes([v]) + seg[at + 1:]))
    # two traks, the one in front with an 'mp4a' entry: through the reader and the two rewriters, at every truncation; its
    # protected form through the un-protector likewise; and the 'mp4a' entry shrunk to 40 bytes, which ends the stsd's walk
    seg = two_tracks("mp4a", True)
    prot = P.init_protect(seg, TENC, PSSH, 5)
    at = seg.index(b"mp4a") - 4
    for kind in (1, 2, 3):
        out += [(kind, dict(track_id=track), seg[:n]) for track in (0, 5) for n in range(len(seg) + 1)]
        out += [(kind, dict(track_id=track), seg[:at] + struct.pack(">I", 40) + seg[at + 4:]) for track in (0, 5, 9)]
    out += [(3, dict(track_id=track), prot[:n]) for track in (0, 5) for n in range(len(prot) + 1)]
    return out


def test_rules_and_init_reader_under_sanitizers(tmp_path):
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
    src = tmp_path / "mp4rd_host_asan.cpp"
    src.write_text(PROGRAM.replace("@TENC@", ", ".join(str(x) for x in TENC.tobytes())).replace("@PSSH@", ", ".join(str(x) for x in PSSH[0])))
    exe = tmp_path / "mp4rd_host_asan"
    cmd = [cxx] + flags + ["-I", os.path.join(ROOT, "hevcbitstream_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    todo = cases()
    with open(tmp_path / "cases.bin", "wb") as f:
        for kind, prm, buf in todo:
            f.write(struct.pack("<5IQ", kind, prm["track_id"], prm.get("trex_duration", 0), prm.get("trex_size", 0), prm.get("trex_flags", 0),
                                len(buf)))
            f.write(buf)
    run = subprocess.run([str(exe), str(tmp_path / "cases.bin")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-6000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(todo)
    verdicts = set()
    for i, ((kind, prm, buf), got) in enumerate(zip(todo, lines)):
        want = (want_samples, want_init, want_protect, want_unprotect)[kind](buf, prm if kind == 0 else prm["track_id"])
        assert got == want, (i, kind, prm, len(buf))
        verdicts.add((kind, got.split()[0]))
    assert verdicts == {(0, "ok"), (0, "big"), (0, "chain"), (0, "moof"), (0, "sample"), (1, "ok"), (1, "refused"), (2, "ok"), (2, "refused"),
                        (3, "ok"), (3, "refused")}
