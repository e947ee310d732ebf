"""The aggregation rule of hbs_rtp.h (rtp_group_next, rtp_ap_fold / rtp_ap_payload_hdr, rtp_ap_head_byte, the flag in
rtp_params_ok) and hbs_rtp_ap_units_host (hbs_rtpun.h) under AddressSanitizer and UBSan, in a stand-alone program: the groups of
hand-computed cases and of random ones against the definition walked one NAL at a time, the head bytes of an AP against bytes
written by hand, and truncated, oversized, empty and nested aggregation packets at the end of exactly sized heap blocks.
Nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "hbs_rtpun.h"

static uint64_t state = 0x7654321ull;
static uint64_t rnd() { state = state * 6364136223846793005ull + 1442695040888963407ull; return state >> 20; }

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "line %d: %s (case %d)\n", __LINE__, #x, c); return 2; } } while (0)

/* the group starts of n NALs by rtp_group_next, span by span, from exactly sized heap tables */
static std::vector<uint32_t> starts_of(const std::vector<uint64_t>& L, const std::vector<uint32_t>& au, uint32_t mp)
{
    std::vector<uint32_t> out;
    const uint64_t n = L.size();
    for (uint64_t base = 0; base < n; base += HBS_RTP_AP_SPAN) {
        const uint32_t hi = (uint32_t)(n - base < HBS_RTP_AP_SPAN ? n - base : HBS_RTP_AP_SPAN);
        uint64_t* pre = (uint64_t*)malloc((hi + 1) * sizeof(uint64_t));
        uint32_t* a = (uint32_t*)malloc(hi * sizeof(uint32_t));
        pre[0] = 0;
        for (uint32_t i = 0; i < hi; ++i) { pre[i + 1] = pre[i] + hbs::rtp_ap_weight(L[base + i]); a[i] = au[base + i]; }
        for (uint32_t i = 0; i < hi; ) {
            out.push_back((uint32_t)base + i);
            const uint32_t next = hbs::rtp_group_next(i, hi, mp, [&](uint32_t j) { return pre[j]; }, [&](uint32_t j) { return a[j]; });
            if (next <= i || next > hi) { out.clear(); free(pre); free(a); return out; }
            i = next;
        }
        free(pre); free(a);
    }
    return out;
}

/* ... and by the definition, one NAL at a time */
static std::vector<uint32_t> starts_plain(const std::vector<uint64_t>& L, const std::vector<uint32_t>& au, uint32_t mp)
{
    std::vector<uint32_t> out;
    const uint64_t n = L.size();
    for (uint64_t i = 0; i < n; ) {
        out.push_back((uint32_t)i);
        uint64_t j = i + 1, sum = 2 + 2 + L[i];
        while (j < n && j % 256 != 0 && au[j] == au[i] && sum + 2 + L[j] <= mp) { sum += 2 + L[j]; ++j; }
        i = j;
    }
    return out;
}

struct Case { uint32_t mp; std::vector<uint64_t> L; std::vector<uint32_t> au; std::vector<uint32_t> starts; };

int main()
{
    int c = 0;
    {   /* the flag */
        hbs_rtp_params prm;
        memset(&prm, 0, sizeof(prm));
        prm.max_payload = 100;
        prm.flags = HBS_RTP_AGGREGATE; CHECK(hbs::rtp_params_ok(&prm));
        prm.flags = HBS_RTP_AGGREGATE | HBS_RTP_OPEN_END; CHECK(hbs::rtp_params_ok(&prm));
        prm.flags = 2; CHECK(!hbs::rtp_params_ok(&prm));
        prm.flags = 6; CHECK(!hbs::rtp_params_ok(&prm));
        prm.flags = 8; CHECK(!hbs::rtp_params_ok(&prm));
        prm.flags = 0x80000004u; CHECK(!hbs::rtp_params_ok(&prm));
        CHECK(HBS_RTP_AGGREGATE == 4u && HBS_RTP_AP_SPAN == 256);
    }
    /* hand-computed groups */
    const Case cases[] = {
        {100, {3, 2, 5}, {0, 0, 0}, {0}},
        {18, {3, 2, 5}, {0, 0, 0}, {0}},                              /* 2 + 5 + 4 + 7 = 18: exactly mp */
        {17, {3, 2, 5}, {0, 0, 0}, {0, 2}},                           /* one byte more than fits */
        {10, {2, 2, 2, 2, 2}, {0, 0, 0, 0, 0}, {0, 2, 4}},
        {9, {2, 2, 2, 2, 2}, {0, 0, 0, 0, 0}, {0, 1, 2, 3, 4}},       /* mp < 10: no AP */
        {4, {2, 2}, {0, 0}, {0, 1}},
        {100, {3, 2, 5, 2}, {7, 7, 8, 8}, {0, 2}},                    /* an AU boundary inside a would-be group */
        {100, {2, 2, 2}, {0, 1, 2}, {0, 1, 2}},                       /* AUs of one NAL */
        {40, {2, 40, 2, 2, 41, 2, 36, 2}, {0, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 4, 5, 6, 7}},
        {100, {2, 92, 2, 2}, {0, 0, 0, 0}, {0, 2}},
        {100, {2, 93, 2, 2}, {0, 0, 0, 0}, {0, 1, 2}},
        {1188, {1ull << 40, 2, 2, 1ull << 62, 2}, {0, 0, 0, 0, 0}, {0, 1, 3, 4}},   /* lengths no packet holds */
    };
    for (c = 0; c < (int)(sizeof(cases) / sizeof(cases[0])); ++c) {
        CHECK(starts_of(cases[c].L, cases[c].au, cases[c].mp) == cases[c].starts);
        CHECK(starts_plain(cases[c].L, cases[c].au, cases[c].mp) == cases[c].starts);
    }
    {   /* 600 NALs of one AU at the largest mp: cut at 256 and 512 and nowhere else */
        c = 100;
        std::vector<uint64_t> L(600, 2);
        std::vector<uint32_t> au(600, 5);
        CHECK((starts_of(L, au, 65523) == std::vector<uint32_t>{0, 256, 512}));
    }
    for (c = 200; c < 600; ++c) {   /* random cases against the definition */
        const uint32_t mps[] = {4, 9, 10, 11, 19, 100, 1188, 65523};
        const uint32_t mp = mps[rnd() % 8];
        const uint64_t n = 1 + rnd() % 700, top = 2 + rnd() % (mp < 100 ? 2 * mp : mp / 3);
        std::vector<uint64_t> L(n);
        std::vector<uint32_t> au(n);
        uint32_t a = (uint32_t)rnd();
        for (uint64_t i = 0; i < n; ++i) { L[i] = 2 + rnd() % top; if (rnd() % 8 == 0) ++a; au[i] = a; }
        CHECK(starts_of(L, au, mp) == starts_plain(L, au, mp));
    }
    {   /* the PayloadHdr */
        c = 700;
        uint32_t acc = hbs::kRtpApFoldStart;
        acc = hbs::rtp_ap_fold(acc, 0x40, 0x01); acc = hbs::rtp_ap_fold(acc, 0xC3, 0xFA); acc = hbs::rtp_ap_fold(acc, 0x4E, 0x09);
        CHECK(hbs::rtp_ap_payload_hdr(acc) == (0xE0u | 0x01u << 8));
        acc = hbs::rtp_ap_fold(hbs::rtp_ap_fold(hbs::kRtpApFoldStart, 0x41, 0x0B), 0x01, 0xFA);      /* layers 33 and 63, tids 3 and 2 */
        CHECK(hbs::rtp_ap_payload_hdr(acc) == (0x61u | 0x0Au << 8));
        acc = hbs::rtp_ap_fold(hbs::rtp_ap_fold(hbs::kRtpApFoldStart, 0x4E, 0x09), 0x02, 0x01);
        CHECK(hbs::rtp_ap_payload_hdr(acc) == (0x60u | 0x01u << 8));
        acc = hbs::rtp_ap_fold(hbs::rtp_ap_fold(hbs::kRtpApFoldStart, 0x01, 0xFF), 0x01, 0xFF);      /* layer 63, tid 7: nothing lower */
        CHECK(hbs::rtp_ap_payload_hdr(acc) == (0x61u | 0xFFu << 8));
    }
    for (int fr = 0; fr <= 2; fr += 2) {   /* every byte in front of an AP's first unit against bytes written by hand */
        c = 800 + fr;
        hbs_rtp_params prm;
        memset(&prm, 0, sizeof(prm));
        prm.max_payload = 100; prm.payload_type = 96; prm.framing = fr; prm.flags = HBS_RTP_AGGREGATE; prm.ssrc = 0xA1B2C3D4u; prm.seq = 0xFFFF;
        const hbs::RtpRule q = hbs::rtp_rule(&prm);
        const uint8_t want[] = {0x00, 0x1E, 0x80, 0xE0, 0x00, 0x01, 0x01, 0x02, 0x03, 0x04, 0xA1, 0xB2, 0xC3, 0xD4, 0xE0, 0x01, 0x01, 0x03};
        const uint32_t head = hbs::rtp_ap_first_head(q);
        CHECK(head == (uint32_t)fr + 16u);
        uint8_t* got = (uint8_t*)malloc(head);
        for (uint32_t i = 0; i < head; ++i) got[i] = (uint8_t)hbs::rtp_ap_head_byte(q, true, 18, 2, 0x01020304u, 0xE0u | 0x01u << 8, 0x0103, i);
        CHECK(memcmp(got, want + (2 - fr), head) == 0);
        got[0] = (uint8_t)hbs::rtp_ap_head_byte(q, false, 18, 2, 0x01020304u, 0xE0u | 0x01u << 8, 0x0103, fr + 1);
        CHECK(got[0] == 0x60);
        free(got);
    }
    {   /* hbs_rtp_ap_units_host: every packet at the end of a heap block of exactly its size */
        c = 900;
        const uint8_t fixed[12] = {0x80, 0x60, 0x02, 0x03, 0x11, 0x22, 0x33, 0x44, 0xA1, 0xB2, 0xC3, 0xD4};
        const uint8_t good[] = {0x60, 0x01, 0x00, 0x02, 0x42, 0x01, 0x00, 0x03, 0x44, 0x01, 0xAA};
        struct Bad { uint8_t b[16]; uint64_t n; };
        const Bad bad[] = {
            {{0x60, 0x01}, 2},                                                        /* empty: no unit */
            {{0x60, 0x01, 0x00}, 3},                                                  /* a byte for a size */
            {{0x60, 0x01, 0x00, 0x01, 0x42}, 5},                                      /* a size below 2 */
            {{0x60, 0x01, 0x00, 0x00}, 4},
            {{0x60, 0x01, 0x00, 0x03, 0x42, 0x01}, 6},                                /* a size beyond what is left */
            {{0x60, 0x01, 0xFF, 0xFF, 0x42, 0x01}, 6},                                /* oversized */
            {{0x60, 0x01, 0x00, 0x02, 0x42, 0x01, 0xFF}, 7},                          /* a byte behind the last unit */
            {{0x60, 0x01, 0x00, 0x02, 0x42, 0x01, 0x00, 0x04, 0x60, 0x01, 0x00, 0x00}, 12},   /* a nested AP */
            {{0x60, 0x01, 0x00, 0x02, 0x62, 0x01}, 6},                                /* an FU inside */
            {{0x42, 0x01, 0xAA}, 3},                                                  /* not an AP */
        };
        uint64_t off[4], size[4];
        for (uint64_t cut = 0; cut <= sizeof(good); ++cut) {                          /* every truncation of a good packet */
            const uint64_t n = 12 + cut;
            uint8_t* p = (uint8_t*)malloc(n);
            memcpy(p, fixed, 12); memcpy(p + 12, good, cut);
            const int64_t rc = hbs::rtp_ap_units_host(p, n, off, size, 4);
            if (cut == sizeof(good)) CHECK(rc == 2 && off[0] == 16 && size[0] == 2 && off[1] == 20 && size[1] == 3);
            else if (cut == 6) CHECK(rc == 1 && off[0] == 16 && size[0] == 2);    /* (the packet of the first unit alone) */
            else CHECK(rc == HBS_E_ARG);
            free(p);
        }
        for (c = 901; c < 901 + (int)(sizeof(bad) / sizeof(bad[0])); ++c) {
            const Bad& b = bad[c - 901];
            uint8_t* p = (uint8_t*)malloc(12 + b.n);
            memcpy(p, fixed, 12); memcpy(p + 12, b.b, b.n);
            CHECK(hbs::rtp_ap_units_host(p, 12 + b.n, off, size, 4) == HBS_E_ARG);
            free(p);
        }
        c = 950;
        uint8_t* p = (uint8_t*)malloc(12 + sizeof(good));
        memcpy(p, fixed, 12); memcpy(p + 12, good, sizeof(good));
        uint64_t* one_off = (uint64_t*)malloc(8);
        uint64_t* one_size = (uint64_t*)malloc(8);
        CHECK(hbs::rtp_ap_units_host(p, 12 + sizeof(good), one_off, one_size, 1) == 2 && *one_off == 16 && *one_size == 2);   /* counted beyond cap */
        CHECK(hbs::rtp_ap_units_host(p, 12 + sizeof(good), nullptr, nullptr, 0) == 2);
        CHECK(hbs::rtp_ap_units_host(p, 12 + sizeof(good), nullptr, nullptr, 1) == HBS_E_ARG);
        CHECK(hbs::rtp_ap_units_host(nullptr, 23, one_off, one_size, 1) == HBS_E_ARG);
        CHECK(hbs::rtp_ap_units_host(p, 11, one_off, one_size, 1) == HBS_E_ARG);
        p[0] = 0xA0; p[12 + sizeof(good) - 1] = 5;                                     /* padding takes the second unit */
        CHECK(hbs::rtp_ap_units_host(p, 12 + sizeof(good), one_off, one_size, 1) == 1);
        free(one_off); free(one_size); free(p);
    }
    printf("groups, head bytes and aggregation packets checked\n");
    return 0;
}
"""


def test_group_rule_head_bytes_and_ap_units_under_sanitizers(tmp_path):
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
    src = tmp_path / "rtp_ap_host_asan.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "rtp_ap_host_asan"
    cmd = [cxx] + flags + ["-I", os.path.join(ROOT, "hevcbitstream_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "aggregation packets checked" in run.stdout
