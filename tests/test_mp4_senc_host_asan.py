"""The host/device rule of hbs_mp4senc.h (mp4senc_find, mp4senc_record, mp4senc_hint_ok, the entry and IV readers, the clear-sample
EMIT) and hbs_mp4_init_unprotect_host under AddressSanitizer and UBSan, in a stand-alone program: protected fragments of 1..40
samples with every iv_size, made through the writer's rule into exactly sized heap blocks and read back through the call's host
loop with a right saiz, a wrong one, a short one and none; every truncation of a fragment; init segments protected, read back
from blocks that end with their allocation, and cut short at every length.  Nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "hbs_mp4senc.h"

static uint64_t state = 0x1234567ull;
static uint64_t rnd() { state = state * 6364136223846793005ull + 1442695040888963407ull; return state >> 20; }

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "line %d: %s (S %u V %u)\n", __LINE__, #x, S, V); return 2; } } while (0)

static uint8_t* exact(const uint8_t* from, uint64_t n)        /* a heap block of exactly n bytes */
{
    uint8_t* p = (uint8_t*)malloc(n ? n : 1);
    if (!n) { free(p); return nullptr; }
    memcpy(p, from, n);
    return p;
}

static bool same(const hbs::SencHostOut& o, const uint64_t* sf, const hbs_cenc_subsample* sub, const uint8_t* iv, uint32_t S, uint32_t V)
{
    if (o.error || o.sub_first.size() != S + 1u || o.sub.size() != sf[S]) return false;
    for (uint32_t s = 0; s <= S; ++s) if (o.sub_first[s] != sf[s]) return false;
    for (uint64_t e = 0; e < sf[S]; ++e) if (o.sub[e].clear != sub[e].clear || o.sub[e].protect != sub[e].protect) return false;
    for (uint32_t i = 0; i < 16 * S; ++i) if (o.iv[i] != (V && i % 16 < V ? iv[i] : 0)) return false;
    return true;
}

int main()
{
    unsigned long fragments = 0, cuts = 0;
    uint32_t S = 0, V = 0;
    /* the small rules */
    {
        const uint8_t two[2] = {0x12, 0x34};
        uint8_t* p = exact(two, 2);
        CHECK(hbs::rd_be16(p, 0) == 0x1234);
        free(p);
        CHECK(hbs::mp4senc_clear_count(0) == 0 && hbs::mp4senc_clear_count(1) == 1 && hbs::mp4senc_clear_count(65535) == 1);
        CHECK(hbs::mp4senc_clear_count(65536) == 2 && hbs::mp4senc_clear_count(200000) == 4);
        CHECK(hbs::mp4senc_clear_entry(65536, 0).clear == 65535 && hbs::mp4senc_clear_entry(65536, 1).clear == 1);
        CHECK(hbs::mp4senc_clear_entry(200000, 3).clear == 200000 - 3 * 65535 && hbs::mp4senc_clear_entry(200000, 3).protect == 0);
        CHECK(hbs::mp4senc_flat_count(0) == 0 && hbs::mp4senc_flat_count(7) == 1);
        CHECK(hbs::mp4prot_numbering_ok(5, 5, 2, 7, true) && !hbs::mp4prot_numbering_ok(5, 5, 2, 8, true) && !hbs::mp4prot_numbering_ok(4, 5, 2, 7, false));
        /* a record that ends with its box, and with the allocation */
        const uint8_t rec[10] = {9, 9, 0, 1, 0, 5, 0, 0, 0, 20};
        uint8_t* r = exact(rec, 10);
        uint32_t n;
        uint64_t next;
        CHECK(hbs::mp4senc_record(r, 0, 10, 2, n, next) && n == 1 && next == 10);
        CHECK(!hbs::mp4senc_record(r, 0, 9, 2, n, next) && !hbs::mp4senc_record(r, 8, 10, 2, n, next) && !hbs::mp4senc_record(r, 10, 10, 2, n, next));
        CHECK(hbs::mp4senc_hint_ok(r, 0, 10, 2, 0, 10, n) && n == 1);
        CHECK(!hbs::mp4senc_hint_ok(r, 0, 10, 2, 0, 16, n) && !hbs::mp4senc_hint_ok(r, 0, 10, 2, 0, 4, n) && !hbs::mp4senc_hint_ok(r, 0, 10, 2, 11, 10, n));
        CHECK(!hbs::mp4senc_hint_ok(r, 0, 10, 2, 8, 2, n) && !hbs::mp4senc_hint_ok(r, 0, 10, 2, 0, 3, n));
        const hbs_cenc_subsample e = hbs::mp4senc_entry(r, 0, 2, 0);
        CHECK(e.clear == 5 && e.protect == 20);
        free(r);
    }
    for (S = 1; S <= 40; ++S) {
        for (V = 0; V <= 16; V += 8) {
            const uint32_t cap = hbs::mp4prot_max_entries(V);
            uint64_t* sf = (uint64_t*)malloc((S + 1) * sizeof(uint64_t));
            sf[0] = 0;
            for (uint32_t s = 0; s < S; ++s) sf[s + 1] = sf[s] + (s == S / 2 ? cap : rnd() % 5);
            const uint64_t E = sf[S];
            hbs_cenc_subsample* sub = (hbs_cenc_subsample*)malloc(E ? E * sizeof(hbs_cenc_subsample) : 1);
            for (uint64_t e = 0; e < E; ++e) { sub[e].clear = (uint32_t)(rnd() % 200 == 0 ? 65535 : rnd() % 40); sub[e].protect = (uint32_t)(rnd() % 90); }
            uint8_t* iv = (uint8_t*)malloc(16 * S);
            for (uint32_t i = 0; i < 16 * S; ++i) iv[i] = (V == 8 && i % 16 >= 8) ? 0 : (uint8_t)(1 + rnd() % 255);
            hbs::Mp4HostSample* hs = (hbs::Mp4HostSample*)malloc(S * sizeof(hbs::Mp4HostSample));
            uint64_t* size = (uint64_t*)malloc(S * sizeof(uint64_t));
            uint64_t P = 0;
            for (uint32_t s = 0; s < S; ++s) {
                uint32_t z = 0;
                for (uint64_t e = sf[s]; e < sf[s + 1]; ++e) z += sub[e].clear + sub[e].protect;
                uint8_t* b = (uint8_t*)malloc(z ? z : 1);
                for (uint32_t i = 0; i < z; ++i) b[i] = (uint8_t)rnd();
                hs[s].sw[0] = (uint32_t)rnd(); hs[s].sw[1] = z; hs[s].sw[2] = hbs::mp4_sample_flags(rnd() & 1); hs[s].sw[3] = (uint32_t)rnd();
                hs[s].bytes = b;
                size[s] = z;
                P += z;
            }
            hbs_mp4_frag f;
            memset(&f, 0, sizeof(f));
            f.samples = S; f.sequence = (uint32_t)rnd(); f.decode_time = rnd(); f.out_bytes = hbs::mp4_fragment_bytes(S, P); f.first_au = 77;
            uint8_t* in = (uint8_t*)malloc(f.out_bytes);
            hbs::mp4_write_fragment_host(f, 3, hs, in);
            const uint64_t total = f.out_bytes + hbs::mp4prot_growth(S, E, V);
            uint8_t* prot = (uint8_t*)malloc(total);
            hbs::mp4prot_write_fragment_host(in, f, V, sf, sub, iv, prot);
            hbs_mp4_frag g = f;
            g.out_off = 0; g.out_bytes = total;
            hbs_mp4_senc_params prm;
            memset(&prm, 0, sizeof(prm));
            prm.iv_size = V;
            CHECK(hbs::mp4_senc_params_ok(&prm));
            hbs::SencHostOut o;
            /* as written: the hint settles the fragment */
            hbs::mp4_senc_samples_host(prot, total, &g, 1, nullptr, S, prm, o);
            CHECK(same(o, sf, sub, iv, S, V) && o.hinted == 1 && o.senc_read == 1);
            prm.track_id = 3;
            hbs::mp4_senc_samples_host(prot, total, &g, 1, size, S, prm, o);
            CHECK(same(o, sf, sub, iv, S, V) && o.hinted == 1);
            prm.track_id = 4;
            hbs::mp4_senc_samples_host(prot, total, &g, 1, size, S, prm, o);
            CHECK(o.error == HBS_E_ARG && o.bad_frag == 1);
            prm.track_id = 0;
            const uint64_t saiz = 88 + 16ull * S;                  /* the saiz box: sample_count at + 13, the sizes at + 17 */
            CHECK(!memcmp(prot + saiz + 4, "saiz", 4));
            /* a wrong saiz (one size byte changed), a short one (its count is another), none: the walk gives the same */
            uint8_t* x = exact(prot, total);
            x[saiz + 17 + S / 2] ^= 6;
            hbs::mp4_senc_samples_host(x, total, &g, 1, nullptr, S, prm, o);
            CHECK(same(o, sf, sub, iv, S, V) && o.hinted == 0);
            memcpy(x, prot, total);
            x[saiz + 16] ^= 1;
            hbs::mp4_senc_samples_host(x, total, &g, 1, nullptr, S, prm, o);
            CHECK(same(o, sf, sub, iv, S, V) && o.hinted == 0);
            memcpy(x, prot, total);
            x[saiz + 3] -= 1;                                       /* the saiz box a byte short, a stray byte behind it */
            hbs::mp4_senc_samples_host(x, total, &g, 1, nullptr, S, prm, o);
            CHECK(o.error == HBS_E_ARG);                            /* (the stray byte breaks the box rule) */
            memcpy(x, prot, total);
            memcpy(x + saiz + 4, "free", 4);
            hbs::mp4_senc_samples_host(x, total, &g, 1, nullptr, S, prm, o);
            CHECK(same(o, sf, sub, iv, S, V) && o.hinted == 0);
            /* the senc renamed: an error, or with the flag wholly clear samples */
            const uint64_t senc = saiz + 17 + S + 20;
            CHECK(!memcmp(x + senc + 4, "senc", 4));
            memcpy(x + senc + 4, "skip", 4);
            hbs::mp4_senc_samples_host(x, total, &g, 1, size, S, prm, o);
            CHECK(o.error == HBS_E_ARG && o.bad_frag == 1);
            prm.flags = HBS_SENC_CLEAR_IF_ABSENT;
            hbs::mp4_senc_samples_host(x, total, &g, 1, size, S, prm, o);
            CHECK(o.error == 0 && o.protect == 0 && o.senc_read == 0);
            for (uint32_t s = 0; s < S; ++s) CHECK(o.sub_first[s + 1] - o.sub_first[s] == hbs::mp4senc_clear_count(size[s]));
            prm.flags = 0;
            free(x);
            /* every truncation, from a block of exactly the bytes that are left: the fragment table says what is there ... */
            const uint64_t moof = hbs::mp4prot_moof_bytes(S, E, V);
            for (uint64_t cut = 0; cut < moof + 8 && S <= 6; ++cut) {
                uint8_t* part = exact(prot, cut);
                hbs_mp4_frag h = g;
                h.out_bytes = cut;
                hbs::mp4_senc_samples_host(part, cut, &h, 1, nullptr, S, prm, o);
                CHECK(cut >= moof ? same(o, sf, sub, iv, S, V) : o.error == HBS_E_ARG);
                /* ... or still says the whole */
                hbs::mp4_senc_samples_host(part, cut, &g, 1, nullptr, S, prm, o);
                CHECK(o.error == HBS_E_ARG && o.bad_frag == 1);
                free(part);
                ++cuts;
            }
            ++fragments;
            for (uint32_t s = 0; s < S; ++s) free((void*)hs[s].bytes);
            free(hs); free(size); free(in); free(prot); free(iv); free(sub); free(sf);
        }
    }
    /* init segments: protected, read back from a block that ends with its allocation, and cut short at every length */
    static const uint8_t vps[] = {0x40, 0x01, 0x0C, 0x01, 0xFF, 0xFF};
    static const uint8_t sps[] = {0x42, 0x01, 0x01, 0x01, 0x60, 0x00, 0x00, 0x03, 0x00, 0x90, 0x00, 0x00, 0x03, 0x00, 0x00, 0x03, 0x00, 0x78, 0xA0};
    static const uint8_t pps[] = {0x44, 0x01, 0xC1, 0x72};
    S = 0;
    for (V = 0; V <= 16; V += 8) {
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
        for (int i = 0; i < 16; ++i) t.kid[i] = (uint8_t)(i + 1);
        if (!V) { t.constant_iv_size = 16; t.crypt_byte_block = 1; t.skip_byte_block = 9; memset(t.constant_iv, 0xA5, 16); }
        static const uint8_t pssh_bytes_[] = {0, 0, 0, 35, 'p', 's', 's', 'h', 0, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 0, 0, 0, 3, 7, 7, 7};
        const uint8_t* boxes[2] = {pssh_bytes_, pssh_bytes_};
        const uint64_t sizes[2] = {sizeof(pssh_bytes_), sizeof(pssh_bytes_)};
        const int64_t need = hbs::mp4_init_protect(init, (uint64_t)n, 3, &t, boxes, sizes, 2, nullptr, 0);
        CHECK(need > n);
        uint8_t* prot = (uint8_t*)malloc((size_t)need);
        CHECK(hbs::mp4_init_protect(init, (uint64_t)n, 3, &t, boxes, sizes, 2, prot, (uint64_t)need) == need);
        hbs_mp4_tenc got;
        uint32_t format = 0;
        uint64_t off[2] = {0, 0}, len[2] = {0, 0}, k = 9;
        uint8_t* out = (uint8_t*)malloc((size_t)n);
        CHECK(hbs_mp4_init_unprotect_host(prot, (uint64_t)need, 0, &got, &format, off, len, 1, &k, out, (uint64_t)n - 1) == n);
        CHECK(k == 2 && len[0] == 35 && len[1] == 0 && !memcmp(prot + off[0], pssh_bytes_, 35));
        CHECK(hbs_mp4_init_unprotect_host(prot, (uint64_t)need, 3, &got, &format, off, len, 2, &k, out, (uint64_t)n) == n);
        CHECK(!memcmp(out, init, (size_t)n) && !memcmp(&got, &t, sizeof(t)) && k == 2 && len[1] == 35 && off[1] == off[0] + 35);
        CHECK(format == (V == 8 ? HBS_MP4_FOURCC('h', 'e', 'v', '1') : HBS_MP4_FOURCC('h', 'v', 'c', '1')));
        CHECK(hbs_mp4_init_unprotect_host(prot, (uint64_t)need, 4, &got, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0) == HBS_E_ARG);
        CHECK(hbs_mp4_init_unprotect_host(init, (uint64_t)n, 0, &got, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0) == HBS_E_ARG);
        CHECK(hbs_mp4_init_unprotect_host(prot, (uint64_t)need, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0) == HBS_E_ARG);
        for (int64_t cut = 0; cut < need; ++cut) {
            uint8_t* part = exact(prot, (uint64_t)cut);
            CHECK(hbs_mp4_init_unprotect_host(part, (uint64_t)cut, 0, &got, &format, off, len, 2, &k, out, (uint64_t)n) == HBS_E_ARG);
            free(part);
            ++cuts;
        }
        free(init); free(prot); free(out);
    }
    if (!fragments || !cuts) { fprintf(stderr, "nothing was driven\n"); return 5; }
    printf("%lu fragments read back, %lu buffers cut short\n", fragments, cuts);
    return 0;
}

extern "C" int64_t hbs_mp4_init_unprotect_host(const uint8_t* init, uint64_t n, uint32_t track_id, hbs_mp4_tenc* t_out, uint32_t* format_out,
                                               uint64_t* pssh_off, uint64_t* pssh_bytes, uint64_t pssh_cap, uint64_t* n_pssh_out, uint8_t* out, uint64_t cap)
{
    return hbs::mp4_init_unprotect(init, n, track_id, t_out, format_out, pssh_off, pssh_bytes, pssh_cap, n_pssh_out, out, cap);
}
"""


def test_rule_and_init_unprotect_under_sanitizers(tmp_path):
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
    src = tmp_path / "mp4_senc_host_asan.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "mp4_senc_host_asan"
    cmd = [cxx] + flags + ["-I", os.path.join(ROOT, "hevcbitstream_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "buffers cut short" in run.stdout
