"""The host/device rule of hbs_mp4.h (mp4_head_word, mp4_frag_byte, mp4_len_byte, the times' rule) and the init segment's builder
under AddressSanitizer and UBSan, in a stand-alone program: fragments of 1..40 samples with every length size, written through
the rule's byte function into exactly sized heap blocks and walked box by box; init segments from exactly sized NAL blocks, with
SPS prefixes of 14 and 15 stripped bytes and prefixes that end in 00 00 03.  Nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "hbs_mp4.h"

static uint64_t state = 0x1234567ull;
static uint64_t rnd() { state = state * 6364136223846793005ull + 1442695040888963407ull; return state >> 20; }
static uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "line %d: %s (S %u L %u)\n", __LINE__, #x, S, L); return 2; } } while (0)

static uint8_t* exact(const uint8_t* from, uint64_t n)        /* a heap block of exactly n bytes */
{
    uint8_t* p = (uint8_t*)malloc(n ? n : 1);
    if (!n) { free(p); return nullptr; }
    memcpy(p, from, n);
    return p;
}

int main()
{
    unsigned long fragments = 0, segments = 0;
    for (uint32_t S = 1; S <= 40; ++S) {
        for (uint32_t L = 1; L <= 4; L += L == 2 ? 2 : 1) {
            hbs::Mp4HostSample* s = (hbs::Mp4HostSample*)malloc(S * sizeof(hbs::Mp4HostSample));
            uint64_t P = 0;
            for (uint32_t e = 0; e < S; ++e) {
                const uint32_t nals = (uint32_t)(rnd() % 4);
                uint32_t lens[3], size = 0;
                for (uint32_t k = 0; k < nals; ++k) { lens[k] = (uint32_t)(rnd() % (L == 1 ? 256 : 700)); size += L + lens[k]; }
                uint8_t* b = (uint8_t*)malloc(size ? size : 1);
                uint32_t at = 0;
                for (uint32_t k = 0; k < nals; ++k) {
                    CHECK(hbs::mp4_len_fits(lens[k], L));
                    for (uint32_t i = 0; i < L; ++i) b[at++] = (uint8_t)hbs::mp4_len_byte(lens[k], L, i);
                    for (uint32_t i = 0; i < lens[k]; ++i) b[at++] = (uint8_t)rnd();
                }
                uint32_t dur, cts;
                const uint64_t dts = rnd() & ((1ull << 61) - 1), next = dts + (rnd() & 0xFFFFFFFFull), pts = dts + (rnd() % 5000);
                CHECK(hbs::mp4_au_times(dts, true, e + 1 == S, next, 777u, true, pts, dur, cts));
                CHECK(dur == (e + 1 == S ? 777u : (uint32_t)(next - dts)) && cts == (uint32_t)(pts - dts));
                s[e].sw[0] = dur; s[e].sw[1] = size; s[e].sw[2] = hbs::mp4_sample_flags(rnd() & 1); s[e].sw[3] = cts;
                s[e].bytes = b;
                P += size;
            }
            hbs_mp4_frag f;
            memset(&f, 0, sizeof(f));
            f.samples = S; f.sequence = (uint32_t)rnd(); f.decode_time = rnd() << 20 | rnd();
            f.out_bytes = hbs::mp4_fragment_bytes(S, P);
            CHECK(f.out_bytes == hbs_mp4_fragment_bytes_host(S, P) && f.out_bytes == 96 + 16ull * S + P);
            const uint32_t track = (uint32_t)rnd() | 1u;
            uint8_t* out = (uint8_t*)malloc(f.out_bytes);                 /* exactly the fragment */
            hbs::mp4_write_fragment_host(f, track, s, out);
            /* the boxes tile their parents */
            CHECK(be32(out) == 88 + 16 * S && !memcmp(out + 4, "moof", 4));
            CHECK(be32(out + 8) == 16 && !memcmp(out + 12, "mfhd", 4) && be32(out + 16) == 0 && be32(out + 20) == f.sequence);
            CHECK(be32(out + 24) == be32(out) - 24 && !memcmp(out + 28, "traf", 4));
            CHECK(be32(out + 32) == 16 && !memcmp(out + 36, "tfhd", 4) && be32(out + 40) == 0x00020000u && be32(out + 44) == track);
            CHECK(be32(out + 48) == 20 && !memcmp(out + 52, "tfdt", 4) && be32(out + 56) == 0x01000000u);
            CHECK(((uint64_t)be32(out + 60) << 32 | be32(out + 64)) == f.decode_time);
            CHECK(be32(out + 68) == be32(out + 24) - 44 && !memcmp(out + 72, "trun", 4) && be32(out + 76) == 0x01000F01u);
            CHECK(be32(out + 80) == S && be32(out + 84) == 96 + 16 * S);
            const uint64_t mdat = 88 + 16ull * S;
            CHECK(be32(out + mdat) == 8 + P && !memcmp(out + mdat + 4, "mdat", 4) && mdat + 8 + P == f.out_bytes);
            uint64_t at = mdat + 8;
            for (uint32_t e = 0; e < S; ++e) {
                const uint8_t* t = out + 88 + 16 * e;
                CHECK(be32(t) == s[e].sw[0] && be32(t + 4) == s[e].sw[1] && be32(t + 8) == s[e].sw[2] && be32(t + 12) == s[e].sw[3]);
                CHECK(s[e].sw[1] == 0 || !memcmp(out + at, s[e].bytes, s[e].sw[1]));
                at += s[e].sw[1];
            }
            CHECK(at == f.out_bytes);
            for (uint32_t e = 0; e < S; ++e) free((void*)s[e].bytes);
            free(s); free(out);
            ++fragments;
        }
    }
    {   /* the times' rule at its edges */
        uint32_t S = 0, L = 0, dur, cts;
        uint64_t t;
        CHECK(hbs::mp4_ruled_dts((1ull << 62) - 1, 0, 5, t) && t == (1ull << 62) - 1);
        CHECK(!hbs::mp4_ruled_dts((1ull << 62) - 1, 1, 1, t) && hbs::mp4_ruled_dts((1ull << 62) - 6, 1, 5, t));
        CHECK(!hbs::mp4_ruled_dts((1ull << 62) - 1, 0xFFFFFFFFull, 0xFFFFFFFFu, t) && hbs::mp4_ruled_dts(0, 0x7FFFFFFFull, 0x7FFFFFFFu, t) && !hbs::mp4_ruled_dts(0, 0x80000000ull, 0x80000000u, t));
        CHECK(!hbs::mp4_au_times(1ull << 62, true, true, 0, 1, false, 0, dur, cts) && !hbs::mp4_au_times(~0ull, true, true, 0, 1, false, 0, dur, cts));
        CHECK(!hbs::mp4_au_times(5, true, false, 4, 1, false, 0, dur, cts) && !hbs::mp4_au_times(5, true, false, 5 + (1ull << 32), 1, false, 0, dur, cts));
        CHECK(hbs::mp4_au_times(5, true, false, 5 + 0xFFFFFFFFull, 1, false, 0, dur, cts) && dur == 0xFFFFFFFFu && cts == 0);
        CHECK(hbs::mp4_au_times(1ull << 31, true, true, 0, 9, true, 0, dur, cts) && dur == 9 && cts == 0x80000000u);
        CHECK(!hbs::mp4_au_times((1ull << 31) + 1, true, true, 0, 9, true, 0, dur, cts));
        CHECK(hbs::mp4_au_times(7, true, true, 0, 9, true, 7 + 0x7FFFFFFFull, dur, cts) && cts == 0x7FFFFFFFu);
        CHECK(!hbs::mp4_au_times(7, true, true, 0, 9, true, 7 + 0x80000000ull, dur, cts) && !hbs::mp4_au_times(7, true, true, 0, 9, true, ~0ull, dur, cts));
        CHECK(!hbs::mp4_len_fits(256, 1) && hbs::mp4_len_fits(255, 1) && !hbs::mp4_len_fits(65536, 2) && hbs::mp4_len_fits(0xFFFFFFFFull, 4) && !hbs::mp4_len_fits(1ull << 32, 4));
    }
    /* init segments: the SPS is 42 01 <b2> then twelve profile bytes, cut to `keep` raw bytes, from exactly sized blocks */
    static const uint8_t vps[] = {0x40, 0x01, 0x0C, 0x01, 0xFF, 0xFF};
    static const uint8_t pps[] = {0x44, 0x01, 0xC1, 0x72};
    for (int k = 0; k < 3000; ++k) {
        uint32_t S = (uint32_t)k, L = 0;
        uint8_t raw[64];
        uint32_t n = 0;
        raw[n++] = 0x42; raw[n++] = 0x01; raw[n++] = (uint8_t)rnd();
        const int zeros = (int)(rnd() % 4);                       /* how zero-heavy the profile bytes are */
        uint8_t rbsp[40];
        uint32_t nr = 3;
        rbsp[0] = raw[0]; rbsp[1] = raw[1]; rbsp[2] = raw[2];
        const uint32_t want_rbsp = 10 + (uint32_t)(rnd() % 12);   /* 10..21 stripped bytes: fewer than 15 is refused */
        while (nr < want_rbsp) rbsp[nr++] = (rnd() % 4 < (uint64_t)zeros) ? 0 : (uint8_t)(rnd() % 4 == 0 ? rnd() % 4 : rnd());
        n = 0;
        int z = 0;
        for (uint32_t i = 0; i < nr; ++i) {
            if (z >= 2 && rbsp[i] <= 3) { raw[n++] = 3; z = 0; }
            raw[n++] = rbsp[i];
            z = rbsp[i] == 0 ? z + 1 : 0;
        }
        if (k % 3 == 0 && z >= 2) raw[n++] = 3;                     /* the NAL ends in 00 00 03 */
        uint8_t pre[15];
        const uint32_t got = hbs::mp4_strip_prefix(raw, n, pre, 15);
        CHECK(got == (nr < 15 ? nr : 15) && !memcmp(pre, rbsp, got));
        const uint8_t* nal[3];
        uint64_t bytes[3];
        uint8_t* blk[3] = {exact(vps, sizeof(vps)), exact(raw, n), exact(pps, sizeof(pps))};
        const int order = k % 3;
        for (int i = 0; i < 3; ++i) { nal[i] = blk[(i + order) % 3]; bytes[i] = (i + order) % 3 == 0 ? sizeof(vps) : (i + order) % 3 == 1 ? n : sizeof(pps); }
        hbs_mp4_init_params p;
        p.track_id = 1 + (uint32_t)(rnd() % 100); p.timescale = 90000; p.width = 1 + (uint32_t)(rnd() % 65535); p.height = 1 + (uint32_t)(rnd() % 65535);
        p.length_size = 1 << (rnd() % 3); p.chroma_format_idc = (int)(rnd() % 4); p.bit_depth_luma = 8 + (int)(rnd() % 8); p.bit_depth_chroma = 8 + (int)(rnd() % 8);
        const int flags = (int)(rnd() & 1);
        const int64_t need = hbs::mp4_init_host(&p, flags, nal, bytes, 3, nullptr, 0);
        if (nr < 15) {
            CHECK(need == HBS_E_ARG);
        } else {
            CHECK(need > 0);
            uint8_t* out = (uint8_t*)malloc((size_t)need);          /* exactly the segment */
            CHECK(hbs::mp4_init_host(&p, flags, nal, bytes, 3, out, (uint64_t)need - 1) == need);
            CHECK(hbs_mp4_init_host(&p, flags, nal, bytes, 3, out, (uint64_t)need) == need);
            CHECK(be32(out) == 24 && !memcmp(out + 4, "ftyp", 4) && be32(out + 24) == (uint64_t)need - 24 && !memcmp(out + 28, "moov", 4));
            /* the hvcC: found by its type, its profile bytes and its last array's end */
            int64_t at = -1;
            for (int64_t i = 0; i + 4 <= need; ++i) if (!memcmp(out + i, "hvcC", 4)) { at = i; break; }
            CHECK(at > 0 && out[at + 4] == 1 && !memcmp(out + at + 5, rbsp + 3, 12));
            CHECK(out[at + 25] == (uint8_t)((((rbsp[2] >> 1) & 7) + 1) << 3 | (rbsp[2] & 1) << 2 | (p.length_size - 1)) && out[at + 26] == 3);
            CHECK(out[at + 27] == (flags ? 0x20 : 0xA0) && be32(out + at - 4) == 8 + 23 + 3 * 5 + sizeof(vps) + n + sizeof(pps));
            free(out);
            ++segments;
        }
        /* a NAL of one byte, a NAL of another type, no SPS */
        bytes[0] = 1;
        CHECK(hbs::mp4_init_host(&p, flags, nal, bytes, 3, nullptr, 0) == HBS_E_ARG);
        CHECK(hbs::mp4_init_host(&p, flags, nal, bytes, 0, nullptr, 0) == HBS_E_ARG);
        for (int i = 0; i < 3; ++i) free(blk[i]);
    }
    if (!segments) { fprintf(stderr, "no init segment was built\n"); return 5; }
    printf("%lu fragments written and walked, %lu init segments\n", fragments, segments);
    return 0;
}

extern "C" uint64_t hbs_mp4_fragment_bytes_host(uint64_t samples, uint64_t sample_bytes) { return hbs::mp4_fragment_bytes(samples, sample_bytes); }
extern "C" int64_t hbs_mp4_init_host(const hbs_mp4_init_params* p, int flags, const uint8_t* const* nal, const uint64_t* nal_bytes, uint64_t n,
                                     uint8_t* out, uint64_t cap) { return hbs::mp4_init_host(p, flags, nal, nal_bytes, n, out, cap); }
"""


def test_rule_and_init_segment_under_sanitizers(tmp_path):
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
    src = tmp_path / "mp4_host_asan.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "mp4_host_asan"
    cmd = [cxx] + flags + ["-I", os.path.join(ROOT, "hevcbitstream_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "init segments" in run.stdout
