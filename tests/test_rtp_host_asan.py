"""The host/device rule of hbs_rtp.h (rtp_nal, rtp_packet_bytes, rtp_head_byte) and both host entry points under
AddressSanitizer and UBSan, in a stand-alone program: every packet of NALs of 2..800 bytes for several max_payload and both
framings, written into exactly sized heap blocks from exactly sized NAL blocks and read back with the receiver's rule; truncated
packets are refused.  Nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "hbs_rtp.h"

static uint64_t state = 0x1234567ull;
static uint64_t rnd() { state = state * 6364136223846793005ull + 1442695040888963407ull; return state >> 20; }

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "line %d: %s (L %llu mp %d framing %d p %llu)\n", __LINE__, #x, (unsigned long long)L, mp, fr, (unsigned long long)p); return 2; } } while (0)

int main()
{
    unsigned long packets = 0, refused = 0;
    const int mps[] = {4, 5, 16, 19, 100, 799, 1188, 65523};
    for (int fr = 0; fr <= 2; fr += 2)
    for (int mi = 0; mi < 8; ++mi) {
        const int mp = mps[mi];
        hbs_rtp_params prm;
        memset(&prm, 0, sizeof(prm));
        prm.max_payload = mp; prm.payload_type = (int)(rnd() % 128); prm.framing = fr; prm.ssrc = (uint32_t)rnd(); prm.seq = (uint32_t)(rnd() % 65536);
        uint64_t L = 0, p = 0;
        CHECK(hbs::rtp_params_ok(&prm));
        const hbs::RtpRule q = hbs::rtp_rule(&prm);
        for (L = 2; L <= 800; ++L) {
            uint8_t* nal = (uint8_t*)malloc(L);                         /* exactly L bytes are valid */
            for (uint64_t i = 0; i < L; ++i) nal[i] = (uint8_t)rnd();
            nal[0] = (uint8_t)(((rnd() % 48) << 1) | (rnd() & 0x81));
            const hbs::RtpNal u = hbs::rtp_nal(L, q.mp, q.fr);
            p = 0;
            CHECK(u.packets == hbs::rtp_nal_packets_host(L, mp) && u.fu == (L > (uint64_t)mp) && (u.packets >= 2) == u.fu);
            const bool marker = (rnd() & 1) != 0;
            const uint64_t j = rnd();
            const uint32_t ts = (uint32_t)rnd();
            uint8_t* back = (uint8_t*)malloc(L);
            uint64_t got = 0, total = 0;
            for (p = 0; p < u.packets; ++p) {
                const uint64_t plen = hbs::rtp_packet_bytes(q, L, u, p);
                CHECK(plen > (uint64_t)fr + 12 && plen - fr - 12 <= (uint64_t)mp);
                CHECK(p + 1 == u.packets || plen == hbs::rtp_full_packet_bytes(q));
                uint8_t* out = (uint8_t*)malloc(plen);
                hbs::rtp_write_packet_host(q, nal, L, p, marker, j + p, ts, out);
                if (fr) CHECK((((uint64_t)out[0] << 8) | out[1]) == plen - 2);
                hbs_rtp_packet* r = (hbs_rtp_packet*)malloc(sizeof(hbs_rtp_packet));
                CHECK(hbs::rtp_packet_host(out + fr, plen - fr, r) == 0);
                CHECK(r->payload_off == 12 && r->payload_len == plen - fr - 12);
                CHECK(r->marker == (marker && p + 1 == u.packets ? 1u : 0u) && r->payload_type == (uint32_t)prm.payload_type);
                CHECK(r->seq == ((prm.seq + (uint32_t)(j + p)) & 0xFFFFu) && r->timestamp == ts && r->ssrc == prm.ssrc);
                CHECK(r->nal_type == ((nal[0] >> 1) & 63) && r->nal_header[0] == nal[0] && r->nal_header[1] == nal[1]);
                if (!u.fu) {
                    CHECK(r->kind == HBS_RTP_SINGLE && r->nal_off == 12 && r->nal_len == L && memcmp(out + fr + 12, nal, L) == 0);
                    memcpy(back, nal, L); got = L;
                } else {
                    CHECK(r->kind == HBS_RTP_FU && r->fu_start == (p == 0 ? 1u : 0u) && r->fu_end == (p + 1 == u.packets ? 1u : 0u));
                    CHECK(r->nal_off == 15 && r->nal_len >= 1 && (p + 1 == u.packets || r->nal_len == (uint64_t)mp - 3));
                    if (p == 0) { back[0] = r->nal_header[0]; back[1] = r->nal_header[1]; got = 2; }
                    CHECK(got + r->nal_len <= L);
                    memcpy(back + got, out + fr + r->nal_off, r->nal_len); got += r->nal_len;
                }
                /* every truncation that cuts into the fields is refused; a shorter payload is another, valid packet */
                for (uint64_t cut = 0; cut < 12; ++cut) {
                    uint8_t* part = (uint8_t*)malloc(cut ? cut : 1);
                    memcpy(part, out + fr, cut);
                    CHECK(hbs::rtp_packet_host(part, cut, r) == HBS_E_ARG);
                    free(part);
                    ++refused;
                }
                if (u.fu) {
                    uint8_t* part = (uint8_t*)malloc(14);
                    memcpy(part, out + fr, 14);
                    CHECK(hbs::rtp_packet_host(part, 14, r) == HBS_E_ARG);
                    free(part);
                    ++refused;
                }
                total += plen;
                free(r); free(out);
                ++packets;
            }
            CHECK(got == L && memcmp(back, nal, L) == 0 && total == u.out_bytes);
            free(back); free(nal);
        }
    }
    {   /* the helpers' own limits, packets with CSRC entries, an extension and padding cut short */
        uint64_t L = 0, p = 0; int mp = 0, fr = 0;
        CHECK(hbs::rtp_nal_packets_host(1, 100) == 0 && hbs::rtp_nal_packets_host(100, 3) == 0 && hbs::rtp_nal_packets_host(100, 65524) == 0);
        CHECK(hbs::rtp_nal_packets_host(~0ull, 4) == ~0ull - 2 && hbs::rtp_nal_packets_host(2, 4) == 1);
        hbs_rtp_params prm;
        memset(&prm, 0, sizeof(prm));
        prm.max_payload = 100;
        CHECK(hbs::rtp_params_ok(&prm) && !hbs::rtp_params_ok(nullptr));
        prm.framing = 1; CHECK(!hbs::rtp_params_ok(&prm)); prm.framing = 2;
        prm.flags = 2; CHECK(!hbs::rtp_params_ok(&prm)); prm.flags = 1;
        prm.seq = 65536; CHECK(!hbs::rtp_params_ok(&prm)); prm.seq = 65535;
        prm.payload_type = 128; CHECK(!hbs::rtp_params_ok(&prm)); prm.payload_type = 127;
        prm.max_payload = 3; CHECK(!hbs::rtp_params_ok(&prm)); prm.max_payload = 65524; CHECK(!hbs::rtp_params_ok(&prm));
        prm.max_payload = 65523; CHECK(hbs::rtp_params_ok(&prm));
        const uint8_t full[] = {0xB2, 0xE0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 1, 1, 1, 1, 2, 2, 2, 2, 0xBE, 0xDE, 0, 1, 9, 9, 9, 9, 0x62, 0x01, 0x53, 0xAA, 0, 0, 3};
        const uint64_t n = sizeof(full);
        hbs_rtp_packet r;
        for (uint64_t cut = 0; cut <= n; ++cut) {
            uint8_t* part = (uint8_t*)malloc(cut ? cut : 1);
            memcpy(part, full, cut);
            const int rc = hbs::rtp_packet_host(part, cut, &r);
            if (cut == n) CHECK(rc == 0 && r.kind == HBS_RTP_FU && r.payload_off == 28 && r.payload_len == 4 && r.nal_off == 31 && r.nal_len == 1 && r.fu_end == 1 && r.nal_type == 19);
            else if (rc == 0) CHECK(cut > 28 && part[cut - 1] >= 1 && part[cut - 1] <= cut - 28);      /* a shorter packet whose last byte happens to count its padding */
            else { CHECK(rc == HBS_E_ARG); ++refused; }
            free(part);
        }
        CHECK(hbs::rtp_packet_host(nullptr, 12, &r) == HBS_E_ARG && hbs::rtp_packet_host(full, n, nullptr) == HBS_E_ARG);
    }
    printf("%lu packets written and read back, %lu truncated packets refused\n", packets, refused);
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
    src = tmp_path / "rtp_host_asan.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "rtp_host_asan"
    cmd = [cxx] + flags + ["-I", os.path.join(ROOT, "hevcbitstream_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "truncated packets refused" in run.stdout
