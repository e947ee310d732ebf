"""The host/device rule of hbs_tsmux.h (tsm_packet, tsm_head_byte) and both host entry points under AddressSanitizer and UBSan,
in a stand-alone program: every packet of AUs of 0..800 bytes in every time form, written into exactly sized heap blocks from
exactly sized ES blocks and read back with the demultiplexer's rule; the PAT / PMT pair for random and refused parameters.
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
#include "hbs_tsmux.h"

static uint64_t state = 0x7654321ull;
static uint64_t rnd() { state = state * 6364136223846793005ull + 1442695040888963407ull; return state >> 20; }

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "line %d: %s (E %llu f %u pcr %d j %llu)\n", __LINE__, #x, (unsigned long long)E, f, (int)pcr, (unsigned long long)j); return 2; } } while (0)

int main()
{
    unsigned long packets = 0, pairs = 0;
    const uint32_t pid = 0x1ABC;
    for (uint64_t E = 0; E <= 800; ++E) {
        uint8_t* es = (uint8_t*)malloc(E ? E : 1);                      /* exactly E bytes are valid */
        if (E == 0) { free(es); es = nullptr; }
        for (uint64_t i = 0; i < E; ++i) es[i] = (uint8_t)rnd();
        for (int form = 0; form < 12; ++form) {
            const uint64_t pts = form % 3 == 0 ? ~0ull : (rnd() & hbs::kTsmTimeMask);
            const uint64_t dts = form % 3 == 2 ? (rnd() & hbs::kTsmTimeMask) : (form & 1) ? pts : ~0ull;
            const uint32_t flags = (form & 4) ? HBS_TSMUX_PCR : 0u;
            const uint64_t lead = (form & 8) ? rnd() : 1234;
            const hbs::TsmAu u = hbs::tsm_au(E, pts, dts, (form & 2) != 0, flags);
            const uint32_t f = u.f;
            const bool pcr = u.pcr;
            uint64_t j = 0;
            CHECK(hbs::tsm_times_ok(pts, dts));
            const uint64_t N = hbs::tsm_au_packets(u);
            CHECK(N == hbs::tsm_au_packets_host(E, f == 0 ? 0 : (int)f - 1, flags != 0));
            uint64_t got = 0;
            for (j = 0; j < N; ++j) {
                uint8_t* out = (uint8_t*)malloc(188);
                const uint32_t cc = (uint32_t)rnd();
                hbs::tsm_write_packet_host(u, es, j, pid, lead, cc, out);
                hbs_ts_packet r;
                CHECK(hbs::ts_packet_host(out, 188, (int)pid, &r) == 0);
                CHECK(r.cls == (j == 0 ? HBS_TS_PES_START : HBS_TS_PAYLOAD));
                CHECK(r.cc == (cc & 15u));
                CHECK(j + 1 == N || j == 0 || r.es_len == 184u);
                CHECK(j + 1 == N || r.es_len > 0 || j == 0);
                CHECK(got + r.es_len <= E && (r.es_len == 0 || memcmp(out + r.es_off, es + got, r.es_len) == 0));
                if (j == 0) {
                    CHECK(r.pts == pts && r.dts == (f == 3 ? dts : pts));
                    CHECK(((r.flags & HBS_TS_RANDOM_ACCESS) != 0) == u.irap && (r.flags & HBS_TS_DATA_ALIGNED));
                    CHECK(((out[5] & 0x10) != 0) == pcr);
                    if (pcr) {
                        const uint64_t base = ((uint64_t)out[6] << 25) | ((uint64_t)out[7] << 17) | ((uint64_t)out[8] << 9) | ((uint64_t)out[9] << 1) | (out[10] >> 7);
                        CHECK(base == (((f == 3 ? dts : pts) - lead) & hbs::kTsmTimeMask) && (out[10] & 0x7F) == 0x7E && out[11] == 0);
                    }
                }
                got += r.es_len;
                free(out);
                ++packets;
            }
            CHECK(got == E);
        }
        free(es);
    }
    {   /* the time rules */
        uint64_t E = 0, j = 0; uint32_t f = 0; bool pcr = false;
        CHECK(!hbs::tsm_times_ok(1ull << 33, ~0ull) && !hbs::tsm_times_ok(5, 1ull << 33) && !hbs::tsm_times_ok(~0ull, 5));
        CHECK(hbs::tsm_times_ok(~0ull, ~0ull) && hbs::tsm_times_ok(hbs::kTsmTimeMask, hbs::kTsmTimeMask));
        CHECK(hbs::tsm_au_packets_host(5, 3, 0) == 0 && hbs::tsm_au_packets_host(5, -1, 1) == 0);
        CHECK(hbs::tsm_au_packets_host(~0ull >> 1, 2, 1) > (1ull << 50));
    }
    for (int k = 0; k < 4000; ++k) {
        uint64_t E = 0, j = (uint64_t)k; uint32_t f = 0; bool pcr = false;
        hbs_ts_mux_params* p = (hbs_ts_mux_params*)malloc(sizeof(hbs_ts_mux_params));
        memset(p, 0, sizeof(*p));
        const int sizes[3] = {188, 192, 204};
        p->packet_bytes = sizes[rnd() % 3]; p->pid = 16 + (int)(rnd() % 8175); p->pmt_pid = 16 + (int)(rnd() % 8175);
        p->program_number = 1 + (int)(rnd() % 65535); p->transport_stream_id = (int)(rnd() % 65536);
        p->flags = (uint32_t)(rnd() % 8); p->cc_es = (uint32_t)(rnd() % 16); p->cc_pat = (uint32_t)(rnd() % 16); p->cc_pmt = (uint32_t)(rnd() % 16);
        p->pcr_lead = rnd();
        const int spoil = (int)(rnd() % 12);
        if (spoil == 0) p->pid = (int)(rnd() % 16);
        if (spoil == 1) p->pmt_pid = 8191 + (int)(rnd() % 5);
        if (spoil == 2) p->reserved = 1 + (uint32_t)rnd() % 7;
        if (spoil == 3) p->packet_bytes = 190;
        if (spoil == 4) p->flags |= 8u << (rnd() % 20);
        if (spoil == 5) p->program_number = (rnd() & 1) ? 0 : 65536 + (int)(rnd() % 100);
        const bool ok = hbs::tsm_params_ok(p);
        CHECK(spoil > 5 || !ok || (spoil == 2 && p->reserved == 0));
        uint8_t* pat = (uint8_t*)malloc(188);
        uint8_t* pmt = (uint8_t*)malloc(188);
        const int rc = hbs::tsm_psi_host(p, pat, pmt);
        CHECK((rc == 0) == ok && (rc == 0 || rc == HBS_E_ARG));
        CHECK(hbs::tsm_psi_host(nullptr, pat, pmt) == HBS_E_ARG && hbs::tsm_psi_host(p, nullptr, pmt) == HBS_E_ARG && hbs::tsm_psi_host(p, pat, nullptr) == HBS_E_ARG);
        if (rc == 0) {
            uint8_t* both = (uint8_t*)malloc(376);
            memcpy(both, pat, 188); memcpy(both + 188, pmt, 188);
            int prog = -1;
            CHECK(hbs::ts_find_pid_host(both, 376, 188, 0x24, &prog) == p->pid && prog == p->program_number);
            CHECK(hbs::tsm_crc32(pat + 5, 16) == 0 && hbs::tsm_crc32(pmt + 5, 27) == 0);
            CHECK((pat[3] & 15u) == p->cc_pat && (pmt[3] & 15u) == p->cc_pmt && pat[187] == 0xFF && pmt[187] == 0xFF);
            free(both);
            ++pairs;
        }
        free(pat); free(pmt); free(p);
    }
    if (!pairs) { fprintf(stderr, "no PAT / PMT pair was built\n"); return 5; }
    printf("%lu packets written and read back, %lu PSI pairs\n", packets, pairs);
    return 0;
}
"""


def test_rule_and_host_functions_under_sanitizers(tmp_path):
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
    src = tmp_path / "tsmux_host_asan.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "tsmux_host_asan"
    cmd = [cxx] + flags + ["-I", os.path.join(ROOT, "hevcbitstream_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "PSI pairs" in run.stdout
