"""The host/device rule of hbs_mp4prot.h (mp4prot_frag_ok, mp4prot_sample_tables, mp4prot_sample_entries, mp4prot_moof_byte) and
hbs_mp4_init_protect_host under AddressSanitizer and UBSan, in a stand-alone program: fragments of 1..40 samples with every
iv_size and 0..42 entries a sample, checked and rewritten through the rule from and into exactly sized heap blocks and walked
box by box; init segments cut short at every length, from exactly sized blocks.  Nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "hbs_mp4prot.h"

static uint64_t state = 0x7654321ull;
static uint64_t rnd() { state = state * 6364136223846793005ull + 1442695040888963407ull; return state >> 20; }
static uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }
static uint32_t be16(const uint8_t* p) { return (uint32_t)p[0] << 8 | p[1]; }

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "line %d: %s (S %u V %u)\n", __LINE__, #x, S, V); return 2; } } while (0)

static uint8_t* exact(const uint8_t* from, uint64_t n)        /* a heap block of exactly n bytes */
{
    uint8_t* p = (uint8_t*)malloc(n ? n : 1);
    if (!n) { free(p); return nullptr; }
    memcpy(p, from, n);
    return p;
}

int main()
{
    unsigned long fragments = 0, cuts = 0;
    for (uint32_t S = 1; S <= 40; ++S) {
        for (uint32_t V = 0; V <= 16; V += 8) {
            const uint32_t cap = hbs::mp4prot_max_entries(V);
            CHECK(V + 2 + 6 * cap <= 255 && V + 2 + 6 * (cap + 1) > 255 && cap <= 42);
            /* the tables: 0 .. cap entries a sample, sample S / 2 with exactly cap */
            uint64_t* sf = (uint64_t*)malloc((S + 1) * sizeof(uint64_t));
            sf[0] = 0;
            for (uint32_t s = 0; s < S; ++s) sf[s + 1] = sf[s] + (s == S / 2 ? cap : rnd() % (cap + 1));
            const uint64_t E = sf[S];
            hbs_cenc_subsample* sub = (hbs_cenc_subsample*)malloc(E ? E * sizeof(hbs_cenc_subsample) : 1);
            for (uint64_t e = 0; e < E; ++e) { sub[e].clear = (uint32_t)(rnd() % 200 == 0 ? 65535 : rnd() % 40); sub[e].protect = (uint32_t)(rnd() % 90); }
            uint8_t* iv = (uint8_t*)malloc(16 * S);
            for (uint32_t i = 0; i < 16 * S; ++i) iv[i] = (V == 8 && i % 16 >= 8) ? 0 : (uint8_t)(1 + rnd() % 255);
            /* the fragment hbs_mp4_fragment writes for samples of those sizes, in a block of exactly its bytes */
            hbs::Mp4HostSample* hs = (hbs::Mp4HostSample*)malloc(S * sizeof(hbs::Mp4HostSample));
            uint64_t P = 0;
            for (uint32_t s = 0; s < S; ++s) {
                uint32_t size = 0;
                for (uint64_t e = sf[s]; e < sf[s + 1]; ++e) size += sub[e].clear + sub[e].protect;
                uint8_t* b = (uint8_t*)malloc(size ? size : 1);
                for (uint32_t i = 0; i < size; ++i) b[i] = (uint8_t)rnd();
                hs[s].sw[0] = (uint32_t)rnd(); hs[s].sw[1] = size; hs[s].sw[2] = hbs::mp4_sample_flags(rnd() & 1); hs[s].sw[3] = (uint32_t)rnd();
                hs[s].bytes = b;
                P += size;
            }
            hbs_mp4_frag f;
            memset(&f, 0, sizeof(f));
            f.samples = S; f.sequence = (uint32_t)rnd(); f.decode_time = rnd(); f.out_bytes = hbs::mp4_fragment_bytes(S, P);
            uint8_t* in = (uint8_t*)malloc(f.out_bytes);
            hbs::mp4_write_fragment_host(f, 1 + (uint32_t)rnd() % 9, hs, in);
            /* the rules hold; one byte less of buffer, another count, an entry more, a sum off by one, a clear of 65536 do not */
            CHECK(hbs::mp4prot_frag_ok(in, f.out_bytes, f));
            {
                uint8_t* less = exact(in, f.out_bytes - 1);
                CHECK(!hbs::mp4prot_frag_ok(less, f.out_bytes - 1, f));
                hbs_mp4_frag g = f;
                g.out_bytes -= 1;
                CHECK(!hbs::mp4prot_frag_ok(less, f.out_bytes - 1, g));
                g = f; g.samples = S - 1;
                CHECK(!hbs::mp4prot_frag_ok(in, f.out_bytes, g));
                g = f; g.samples = S + 1;
                CHECK(!hbs::mp4prot_frag_ok(in, f.out_bytes, g));
                g = f; g.out_off = 1;
                CHECK(!hbs::mp4prot_frag_ok(in, f.out_bytes, g));
                g = f; g.out_off = ~0ull;
                CHECK(!hbs::mp4prot_frag_ok(in, f.out_bytes, g));
                free(less);
                const uint32_t at[4] = {76, 80, 84, 88 + 16 * S};
                for (int k = 0; k < 4; ++k) { in[at[k] + 3] ^= 1; CHECK(!hbs::mp4prot_frag_ok(in, f.out_bytes, f)); in[at[k] + 3] ^= 1; }
            }
            for (uint32_t s = 0; s < S; ++s) {
                CHECK(hbs::mp4prot_sample_tables(sf, iv, V, s));
                CHECK(hbs::mp4prot_sample_entries(sub, sf[s], (uint32_t)(sf[s + 1] - sf[s]), hs[s].sw[1]));
                CHECK(!hbs::mp4prot_sample_entries(sub, sf[s], (uint32_t)(sf[s + 1] - sf[s]), hs[s].sw[1] + 1));
            }
            {
                uint64_t t3[3] = {0, cap, 2ull * cap + 1};                              /* cap entries, then cap + 1 */
                uint8_t* iv2 = (uint8_t*)calloc(32, 1);
                CHECK(hbs::mp4prot_sample_tables(t3, iv2, V, 0) && !hbs::mp4prot_sample_tables(t3, iv2, V, 1));
                t3[2] = cap - 1;                                                       /* falling */
                CHECK(!hbs::mp4prot_sample_tables(t3, iv2, V, 1));
                t3[0] = 1;                                                             /* does not start at 0 */
                CHECK(!hbs::mp4prot_sample_tables(t3, iv2, V, 0));
                t3[0] = (1ull << 48) - 1; t3[1] = 1ull << 48; t3[2] = (1ull << 48) + 1;
                CHECK(!hbs::mp4prot_sample_tables(t3 + 1, iv2, V, 0) && !hbs::mp4prot_sample_tables(t3, iv2, V, 1));
                t3[0] = 0; t3[1] = 1; t3[2] = 2;
                iv2[15] = 1;                                                           /* an IV tail, which only 8-byte IVs forbid */
                CHECK(hbs::mp4prot_sample_tables(t3, iv2, V, 0) == (V != 8) && hbs::mp4prot_sample_tables(t3, iv2, V, 1));
                free(iv2);
                if (E) {
                    const uint32_t keep = sub[0].clear;
                    sub[0].clear = 65536;
                    CHECK(!hbs::mp4prot_sample_entries(sub, 0, 1, 65536 + sub[0].protect));
                    sub[0].clear = 65535;
                    CHECK(hbs::mp4prot_sample_entries(sub, 0, 1, 65535 + sub[0].protect));
                    sub[0].clear = keep;
                }
            }
            /* the protected fragment, into a block of exactly its bytes, and walked */
            const uint64_t M = hbs::mp4prot_moof_bytes(S, E, V), total = f.out_bytes + hbs::mp4prot_growth(S, E, V);
            CHECK(total == f.out_bytes + hbs_mp4_protect_bytes_host(S, E, V) && M == 141 + (19 + V) * S + 6 * E);
            uint8_t* out = (uint8_t*)malloc(total);
            hbs::mp4prot_write_fragment_host(in, f, V, sf, sub, iv, out);
            CHECK(be32(out) == M && !memcmp(out + 4, "moof", 4) && !memcmp(out + 8, in + 8, 16));
            CHECK(be32(out + 24) == M - 24 && !memcmp(out + 28, "traf", 4) && !memcmp(out + 32, in + 32, 36));
            CHECK(be32(out + 68) == 20 + 16 * S && !memcmp(out + 72, in + 72, 12) && be32(out + 84) == M + 8 && !memcmp(out + 88, in + 88, 16 * S));
            const uint8_t* saiz = out + 88 + 16 * S;
            CHECK(be32(saiz) == 17 + S && !memcmp(saiz + 4, "saiz", 4) && be32(saiz + 8) == 0 && saiz[12] == 0 && be32(saiz + 13) == S);
            const uint8_t* saio = saiz + 17 + S;
            CHECK(be32(saio) == 20 && !memcmp(saio + 4, "saio", 4) && be32(saio + 8) == 0 && be32(saio + 12) == 1);
            const uint8_t* senc = saio + 20;
            CHECK(be32(senc) == 16 + (V + 2) * S + 6 * E && !memcmp(senc + 4, "senc", 4) && be32(senc + 8) == 2 && be32(senc + 12) == S);
            CHECK(senc + be32(senc) == out + M && out + be32(saio + 16) == senc + 16);
            const uint8_t* aux = out + be32(saio + 16);                 /* found as a player finds it */
            for (uint32_t s = 0; s < S; ++s) {
                const uint32_t n = (uint32_t)(sf[s + 1] - sf[s]);
                CHECK(saiz[17 + s] == V + 2 + 6 * n && !memcmp(aux, iv + 16 * s, V) && be16(aux + V) == n);
                for (uint32_t e = 0; e < n; ++e)
                    CHECK(be16(aux + V + 2 + 6 * e) == sub[sf[s] + e].clear && be32(aux + V + 4 + 6 * e) == sub[sf[s] + e].protect);
                aux += saiz[17 + s];
            }
            CHECK(aux == out + M && !memcmp(out + M, in + 88 + 16 * S, 8 + P) && M + 8 + P == total);
            for (uint32_t s = 0; s < S; ++s) free((void*)hs[s].bytes);
            free(hs); free(in); free(out); free(sf); free(sub); free(iv);
            ++fragments;
        }
    }
    {   /* the numbering rule and the sizes at their edges */
        uint32_t S = 0, V = 0;
        CHECK(hbs::mp4prot_numbering_ok(0, 0, 0, 0, true) && hbs::mp4prot_numbering_ok(5, 5, 3, 8, true) && !hbs::mp4prot_numbering_ok(5, 5, 3, 9, true));
        CHECK(hbs::mp4prot_numbering_ok(5, 5, 3, 9, false) && !hbs::mp4prot_numbering_ok(5, 5, 5, 9, false) && !hbs::mp4prot_numbering_ok(4, 5, 3, 9, false));
        CHECK(!hbs::mp4prot_numbering_ok(~0ull, ~0ull, 2, 9, false));
        CHECK(hbs::mp4prot_moof_bytes(61356671, 0, 16) <= hbs::kProtMoofMax && hbs::mp4prot_moof_bytes(61356672, 0, 16) > hbs::kProtMoofMax);
        CHECK(hbs::mp4prot_moof_bytes(1, 42, 0) == 141 + 19 + 252 && hbs::kProtMoofMax == 2147483639ull);
    }
    /* init segments: cut short at every length, each cut in a block of exactly its bytes */
    static const uint8_t vps[] = {0x40, 0x01, 0x0C, 0x01, 0xFF, 0xFF};
    static const uint8_t sps[] = {0x42, 0x01, 0x01, 0x01, 0x60, 0x00, 0x00, 0x03, 0x00, 0x90, 0x00, 0x00, 0x03, 0x00, 0x00, 0x03, 0x00, 0x78, 0xA0};
    static const uint8_t pps[] = {0x44, 0x01, 0xC1, 0x72};
    for (uint32_t V = 0; V <= 16; V += 8) {
        uint32_t S = 0;
        const uint8_t* nal[3] = {vps, sps, pps};
        const uint64_t bytes[3] = {sizeof(vps), sizeof(sps), sizeof(pps)};
        hbs_mp4_init_params p;
        p.track_id = 3; p.timescale = 90000; p.width = 640; p.height = 360; p.length_size = 4; p.chroma_format_idc = 1; p.bit_depth_luma = 8; p.bit_depth_chroma = 8;
        const int64_t n = hbs::mp4_init_host(&p, V == 8 ? 1 : 0, nal, bytes, 3, nullptr, 0);
        CHECK(n > 0);
        uint8_t* init = (uint8_t*)malloc((size_t)n);
        CHECK(hbs::mp4_init_host(&p, V == 8 ? 1 : 0, nal, bytes, 3, init, (uint64_t)n) == n);
        hbs_mp4_tenc t;
        memset(&t, 0, sizeof(t));
        t.scheme = V ? hbs::kTencCenc : hbs::kTencCbcs; t.iv_size = (uint8_t)V;
        if (!V) { t.constant_iv_size = 16; t.crypt_byte_block = 1; t.skip_byte_block = 9; }
        static const uint8_t pssh_bytes_[] = {0, 0, 0, 35, 'p', 's', 's', 'h', 0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 0, 0, 0, 3, 7, 7, 7};
        uint8_t* box = exact(pssh_bytes_, sizeof(pssh_bytes_));
        const uint8_t* boxes[2] = {box, box};
        const uint64_t sizes[2] = {sizeof(pssh_bytes_), sizeof(pssh_bytes_)};
        for (int64_t cut = 0; cut < n; ++cut) {
            uint8_t* part = exact(init, (uint64_t)cut);
            CHECK(hbs_mp4_init_protect_host(part, (uint64_t)cut, 0, &t, boxes, sizes, 2, nullptr, 0) == HBS_E_ARG);
            free(part);
            ++cuts;
        }
        const uint64_t sinf = 8 + 12 + 20 + 8 + 8 + 24 + (V ? 0 : 17);
        const int64_t need = hbs_mp4_init_protect_host(init, (uint64_t)n, 3, &t, boxes, sizes, 2, nullptr, 0);
        CHECK(need == n + (int64_t)sinf + 70);
        uint8_t* out = (uint8_t*)malloc((size_t)need);
        CHECK(hbs_mp4_init_protect_host(init, (uint64_t)n, 0, &t, boxes, sizes, 2, out, (uint64_t)need - 1) == need);
        CHECK(hbs_mp4_init_protect_host(init, (uint64_t)n, 0, &t, boxes, sizes, 2, out, (uint64_t)need) == need);
        CHECK(be32(out) == 24 && be32(out + 24) == be32(init + 24) + sinf + 70 && !memcmp(out + 28, "moov", 4) && be32(out + 24) == (uint64_t)need - 24);
        CHECK(!memcmp(out + need - 35, pssh_bytes_, 35) && !memcmp(out + need - 70, pssh_bytes_, 35));
        int64_t at = -1;
        for (int64_t i = 0; i + 4 <= need; ++i) if (!memcmp(out + i, "encv", 4)) { at = i; break; }
        CHECK(at > 0 && !memcmp(init + at, V == 8 ? "hev1" : "hvc1", 4) && be32(out + at - 4) == be32(init + at - 4) + sinf);
        const uint8_t* s = out + at - 4 + be32(init + at - 4);
        CHECK(be32(s) == sinf && !memcmp(s + 4, "sinf", 4) && !memcmp(s + 16, init + at, 4) && be32(s + 32) == t.scheme);
        /* one pssh box cut short, or one byte more than its size field says */
        uint8_t* less = exact(pssh_bytes_, sizeof(pssh_bytes_) - 1);
        const uint8_t* bad[1] = {less};
        uint64_t bad_size[1] = {sizeof(pssh_bytes_) - 1};
        CHECK(hbs_mp4_init_protect_host(init, (uint64_t)n, 0, &t, bad, bad_size, 1, nullptr, 0) == HBS_E_ARG);
        bad_size[0] = 7;
        CHECK(hbs_mp4_init_protect_host(init, (uint64_t)n, 0, &t, bad, bad_size, 1, nullptr, 0) == HBS_E_ARG);
        free(less); free(box); free(init); free(out);
    }
    if (!fragments || !cuts) { fprintf(stderr, "nothing was driven\n"); return 5; }
    printf("%lu fragments protected and walked, %lu init segments cut short\n", fragments, cuts);
    return 0;
}

extern "C" uint64_t hbs_mp4_protect_bytes_host(uint64_t samples, uint64_t entries, uint32_t iv_size) { return hbs::mp4prot_growth(samples, entries, iv_size); }
extern "C" int64_t hbs_mp4_init_protect_host(const uint8_t* init, uint64_t n, uint32_t track_id, const hbs_mp4_tenc* t, const uint8_t* const* pssh,
                                             const uint64_t* pssh_bytes, uint64_t n_pssh, uint8_t* out, uint64_t cap)
{
    return hbs::mp4_init_protect(init, n, track_id, t, pssh, pssh_bytes, n_pssh, out, cap);
}
"""


def test_rule_and_init_protect_under_sanitizers(tmp_path):
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
    src = tmp_path / "mp4_protect_host_asan.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "mp4_protect_host_asan"
    cmd = [cxx] + flags + ["-I", os.path.join(ROOT, "hevcbitstream_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "init segments cut short" in run.stdout
