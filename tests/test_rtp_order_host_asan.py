"""The host/device rule of hbs_rtpord.h (rtpo_params_ok, rtpo_read, rtpo_sext16, rtpo_first_ext, rtpo_step, rtpo_late, rtpo_span)
under AddressSanitizer and UBSan, in a stand-alone program: every field the params check refuses, the class of packets with CSRC
entries, an extension and padding in exactly sized heap blocks and truncated by 1..all bytes, the extended sequence numbers at
the differences 0x7FFF / 0x8000 / 0xFFFF, and the start behind after_ext.  Nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "hbs_rtpord.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "line %d: %s (form %d cut %llu)\n", __LINE__, #x, form, (unsigned long long)cut); return 2; } } while (0)

static unsigned long reads = 0, faults = 0, shorter = 0;

/* the packet in a heap block of exactly n bytes */
static hbs::RtpoPacket read_exact(const uint8_t* pkt, uint64_t n, const hbs::RtpoRule& q)
{
    uint8_t* block = (uint8_t*)malloc(n ? n : 1);
    memcpy(block, pkt, n);
    const hbs::RtpoPacket r = hbs::rtpo_read(hbs::RtpBytesAt{block}, n, q);
    ++reads;
    free(block);
    return r;
}

int main()
{
    int form = 0;
    uint64_t cut = 0;
    const uint64_t K = 1ull << 48;

    /* the params check: every refused field */
    hbs_rtp_order_params op;
    memset(&op, 0, sizeof(op));
    op.payload_type = 96; op.max_span = 1000;
    CHECK(hbs::rtpo_params_ok(&op) && !hbs::rtpo_params_ok(nullptr));
    op.payload_type = 128; CHECK(!hbs::rtpo_params_ok(&op)); op.payload_type = -1; CHECK(!hbs::rtpo_params_ok(&op));
    op.payload_type = 0; CHECK(hbs::rtpo_params_ok(&op)); op.payload_type = 127; CHECK(hbs::rtpo_params_ok(&op));
    op.flags = 4; CHECK(!hbs::rtpo_params_ok(&op)); op.flags = 0x80000001u; CHECK(!hbs::rtpo_params_ok(&op));
    op.flags = HBS_RTPO_MATCH_SSRC; CHECK(hbs::rtpo_params_ok(&op));
    op.reserved = 1; CHECK(!hbs::rtpo_params_ok(&op)); op.reserved = 0;
    op.max_span = 0; CHECK(!hbs::rtpo_params_ok(&op)); op.max_span = (1ull << 33) + 1; CHECK(!hbs::rtpo_params_ok(&op));
    op.max_span = ~0ull; CHECK(!hbs::rtpo_params_ok(&op));
    op.max_span = 1ull << 33; CHECK(hbs::rtpo_params_ok(&op)); op.max_span = 1; CHECK(hbs::rtpo_params_ok(&op));
    op.after_ext = 5; CHECK(hbs::rtpo_params_ok(&op));                          /* not read without the flag */
    op.flags = HBS_RTPO_MATCH_SSRC | HBS_RTPO_AFTER;
    CHECK(!hbs::rtpo_params_ok(&op)); op.after_ext = K - 1; CHECK(!hbs::rtpo_params_ok(&op));
    op.after_ext = (1ull << 62) + 1; CHECK(!hbs::rtpo_params_ok(&op)); op.after_ext = ~0ull; CHECK(!hbs::rtpo_params_ok(&op));
    op.after_ext = 1ull << 62; CHECK(hbs::rtpo_params_ok(&op)); op.after_ext = K; CHECK(hbs::rtpo_params_ok(&op));
    op.ssrc = 0xCAFE0001u; op.after_ext = K + 70000;
    const hbs::RtpoRule q = hbs::rtpo_rule(&op);
    CHECK(q.pt == 127 && q.ssrc == 0xCAFE0001u && q.match_ssrc == 1 && q.after == 1 && q.after_ext == K + 70000 && q.max_span == 1);
    op.flags = 0;
    const hbs::RtpoRule plain = hbs::rtpo_rule(&op);
    CHECK(plain.match_ssrc == 0 && plain.after == 0 && plain.after_ext == 0);

    /* sext16 and the ext step */
    CHECK(hbs::rtpo_sext16(0) == 0 && hbs::rtpo_sext16(0x7FFF) == 0x7FFF && hbs::rtpo_sext16(0x8000) == (uint64_t)-32768ll);
    CHECK(hbs::rtpo_sext16(0xFFFF) == (uint64_t)-1ll && hbs::rtpo_sext16(0x12345678FFFEull) == (uint64_t)-2ll && hbs::rtpo_sext16(~0ull) == (uint64_t)-1ll);
    CHECK(hbs::rtpo_step(0, 0x7FFF) == 0x7FFF && hbs::rtpo_step(0, 0x8000) == (uint64_t)-32768ll && hbs::rtpo_step(0, 0xFFFF) == (uint64_t)-1ll);
    CHECK(hbs::rtpo_step(0xFFFF, 0) == 1 && hbs::rtpo_step(0xFFFE, 1) == 3 && hbs::rtpo_step(1, 0xFFFE) == (uint64_t)-3ll && hbs::rtpo_step(7, 7) == 0);
    CHECK(hbs::rtpo_step(0x8001, 0) == 0x7FFF && hbs::rtpo_step(0x8000, 0) == (uint64_t)-32768ll && hbs::rtpo_step(0x1234, 0x9234) == (uint64_t)-32768ll);
    for (uint32_t a = 0; a < 65536; a += 257)
        for (uint32_t d = 0; d < 65536; d += 251) {
            const uint64_t step = hbs::rtpo_step(a, (a + d) & 0xFFFFu);
            CHECK(step == (d < 0x8000u ? (uint64_t)d : (uint64_t)d - 65536u));
            CHECK(((K + a + step) & 0xFFFFu) == ((a + d) & 0xFFFFu));
        }
    /* the first packet: 2^48 + seq, or the number nearest to after_ext with that seq, 32768 below it at the most */
    CHECK(hbs::rtpo_first_ext(plain, 0) == K && hbs::rtpo_first_ext(plain, 0xFFFF) == K + 0xFFFF);
    {
        hbs::RtpoRule r = q;
        const uint64_t afters[] = {K, K + 1, K + 0x7FFF, K + 0x8000, K + 0xFFFF, K + 3 * 65536 + 65534, 1ull << 62};
        for (int i = 0; i < 7; ++i) {
            r.after_ext = afters[i];
            for (uint32_t s = 0; s < 65536; s += 1 + (s > 300 && s < 65000 ? 97 : 0)) {
                const uint64_t e = hbs::rtpo_first_ext(r, s);
                CHECK((e & 0xFFFFu) == s && e + 32768 >= r.after_ext && e <= r.after_ext + 32767);
                CHECK(hbs::rtpo_late(r, e) == (e <= r.after_ext) && !hbs::rtpo_late(plain, e));
            }
            CHECK(hbs::rtpo_first_ext(r, (uint32_t)(r.after_ext & 0xFFFFu)) == r.after_ext);
            CHECK(hbs::rtpo_first_ext(r, (uint32_t)((r.after_ext + 1) & 0xFFFFu)) == r.after_ext + 1);
            CHECK(hbs::rtpo_first_ext(r, (uint32_t)((r.after_ext + 0x8000) & 0xFFFFu)) == r.after_ext - 0x8000);
            CHECK(hbs::rtpo_base(r, r.after_ext + 9) == r.after_ext + 1 && hbs::rtpo_span(r, 1, r.after_ext + 9, r.after_ext + 9) == 9);
            CHECK(hbs::rtpo_span(r, 0, ~0ull, 0) == 0);
        }
        CHECK(hbs::rtpo_base(plain, K + 9) == K + 9 && hbs::rtpo_span(plain, 2, K + 9, K + 12) == 4 && hbs::rtpo_span(plain, 0, ~0ull, 0) == 0);
        CHECK(hbs::rtpo_blocks(0) == 0 && hbs::rtpo_blocks(1) == 1 && hbs::rtpo_blocks(256) == 1 && hbs::rtpo_blocks(257) == 2);
    }

    /* the class of a packet: the four header forms, whole and cut short by 1 .. all bytes */
    hbs::RtpoRule any = plain;
    any.pt = 96;
    hbs::RtpoRule mine = any;
    mine.match_ssrc = 1; mine.ssrc = 0xCAFE0001u;
    for (form = 0; form < 8; ++form) {
        uint8_t buf[128];
        uint64_t n = 12;
        memset(buf, 0, sizeof(buf));
        const uint32_t csrc = form & 1 ? 3u : 0u, ext_words = form & 2 ? 2u : 0u, pad = form & 4 ? 5u : 0u;
        buf[0] = (uint8_t)(0x80 | csrc | (form & 2 ? 0x10 : 0) | (pad ? 0x20 : 0)); buf[1] = 96;
        buf[2] = 0xAB; buf[3] = 0xCD;
        buf[8] = 0xCA; buf[9] = 0xFE; buf[10] = 0x00; buf[11] = 0x01;
        n += 4 * csrc;
        if (form & 2) { buf[n] = 0xBE; buf[n + 1] = 0xDE; buf[n + 2] = 0; buf[n + 3] = (uint8_t)ext_words; n += 4 + 4 * ext_words; }
        const uint64_t head = n;
        buf[n++] = 0x62; buf[n++] = 1; buf[n++] = 0x80 | 19; buf[n++] = 0x55;       /* a fragmentation unit */
        if (pad) { n += pad; buf[n - 1] = (uint8_t)pad; }
        cut = 0;
        hbs::RtpoPacket r = read_exact(buf, n, any);
        CHECK(r.cls == hbs::kRtpoAccepted && r.seq == 0xABCD);
        CHECK(read_exact(buf, n, mine).cls == hbs::kRtpoAccepted);
        buf[1] ^= 1; CHECK(read_exact(buf, n, any).cls == hbs::kRtpoOther); buf[1] ^= 1;
        buf[1] |= 0x80; CHECK(read_exact(buf, n, any).cls == hbs::kRtpoAccepted); buf[1] &= 0x7F;          /* the marker is not the type */
        buf[11] ^= 1; CHECK(read_exact(buf, n, mine).cls == hbs::kRtpoOther && read_exact(buf, n, any).cls == hbs::kRtpoAccepted); buf[11] ^= 1;
        buf[0] ^= 0xC0; CHECK(read_exact(buf, n, any).cls == hbs::kRtpoFault); buf[0] ^= 0xC0;               /* version 1 */
        for (cut = 1; cut <= n; ++cut) {
            const hbs::RtpoPacket t = read_exact(buf, n - cut, any);
            if (t.cls == hbs::kRtpoFault) { CHECK(n - cut < head + 3 + pad || pad); ++faults; }
            else { CHECK(n - cut >= 12 && t.cls == hbs::kRtpoAccepted && t.seq == 0xABCD); ++shorter; }
            if (n - cut < 12) CHECK(t.cls == hbs::kRtpoFault);
        }
    }
    form = 0; cut = 0;
    printf("%lu packets read, %lu truncated packets refused, %lu read as shorter packets\n", reads, faults, shorter);
    return 0;
}
"""


def test_rule_under_sanitizers(tmp_path):
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
    src = tmp_path / "rtp_order_host_asan.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "rtp_order_host_asan"
    cmd = [cxx] + flags + ["-I", os.path.join(ROOT, "hevcbitstream_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "truncated packets refused" in run.stdout
