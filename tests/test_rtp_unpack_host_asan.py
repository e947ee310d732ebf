"""The host/device rule of hbs_rtpun.h (rtpu_read, rtpu_ap_walk, rtpu_continues, rtpu_literal) and hbs_rtp_frames_host's
rtp_frames_host under AddressSanitizer and UBSan, in a stand-alone program: every packet of NALs of 2..400 bytes for several
payload sizes, aggregation packets of 1..8 units, and each of them truncated by 1..all bytes, all in exactly sized heap blocks.
A truncated packet comes back as a fault or as a shorter valid packet, never as a read outside its block.  Nothing is loaded
into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "hbs_rtpun.h"

static uint64_t state = 0x7654321ull;
static uint64_t rnd() { state = state * 6364136223846793005ull + 1442695040888963407ull; return state >> 20; }

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "line %d: %s (L %llu mp %d p %llu cut %llu)\n", __LINE__, #x, (unsigned long long)L, mp, (unsigned long long)p, (unsigned long long)cut); return 2; } } while (0)

static unsigned long reads = 0, faults = 0, shorter = 0;

/* the packet in a heap block of exactly n bytes, through the whole rule: class, and the units of an aggregation packet */
static hbs::RtpuPacket read_exact(const uint8_t* pkt, uint64_t n, const hbs::RtpuRule& q, uint64_t* units, uint64_t* bytes)
{
    uint8_t* block = (uint8_t*)malloc(n ? n : 1);
    memcpy(block, pkt, n);
    hbs::RtpuPacket r = hbs::rtpu_read(hbs::RtpBytesAt{block}, n, q);
    *units = *bytes = 0;
    if (r.cls == hbs::kRtpuAp) {
        uint64_t last_end = 0;
        const bool ok = hbs::rtpu_ap_walk(hbs::RtpBytesAt{block}, r.pay_off, r.pay_len, *units, *bytes,
                                          [&](uint64_t at, uint64_t len) { if (at + len > n || len < 2 || at < last_end) abort(); last_end = at + len; (void)block[at + len - 1]; });
        if (!ok) r.cls = hbs::kRtpuFault;
    }
    if (r.cls != hbs::kRtpuFault && (r.pay_off + r.pay_len + r.pad != n || r.pay_off < 12)) abort();
    ++reads;
    free(block);
    return r;
}

int main()
{
    uint64_t L = 0, p = 0, cut = 0;
    int mp = 0;
    hbs_rtp_unpack_params up;
    memset(&up, 0, sizeof(up));
    up.payload_type = 96; up.startcode_bytes = 4; up.flags = HBS_RTPU_MATCH_SSRC; up.ssrc = 0xCAFE0001u;
    CHECK(hbs::rtpu_params_ok(&up) && !hbs::rtpu_params_ok(nullptr));
    up.startcode_bytes = 5; CHECK(!hbs::rtpu_params_ok(&up)); up.startcode_bytes = 3;
    up.flags = 2; CHECK(!hbs::rtpu_params_ok(&up)); up.flags = HBS_RTPU_MATCH_SSRC;
    up.payload_type = 128; CHECK(!hbs::rtpu_params_ok(&up)); up.payload_type = -1; CHECK(!hbs::rtpu_params_ok(&up)); up.payload_type = 96;
    const hbs::RtpuRule q = hbs::rtpu_rule(&up);
    CHECK(q.sc == 3 && q.match_ssrc == 1 && q.pt == 96);
    CHECK(hbs::rtpu_literal(4, false, 0, 0, 0) == ((4ull << 56) | 0x01000000ull) && hbs::rtpu_literal(3, false, 0, 0, 0) == ((3ull << 56) | 0x010000ull));
    CHECK(hbs::rtpu_literal(4, true, 0xE3, 19, 0x07) == ((6ull << 56) | 0x01000000ull | (0xA7ull << 32) | (0x07ull << 40)));
    CHECK(hbs::rtpu_literal(3, true, 0x62, 1, 0x01) == ((5ull << 56) | 0x010000ull | (0x02ull << 24) | (0x01ull << 32)));

    /* every packet hbs_rtp_pack's rule writes, read, chained and cut short */
    const int mps[] = {4, 5, 19, 60, 399};
    for (int mi = 0; mi < 5; ++mi) {
        mp = mps[mi];
        hbs_rtp_params prm;
        memset(&prm, 0, sizeof(prm));
        prm.max_payload = mp; prm.payload_type = 96; prm.ssrc = up.ssrc; prm.seq = 65530;
        const hbs::RtpRule w = hbs::rtp_rule(&prm);
        uint64_t j = 0;
        for (L = 2; L <= 400; ++L) {
            uint8_t* nal = (uint8_t*)malloc(L);
            for (uint64_t i = 0; i < L; ++i) nal[i] = (uint8_t)rnd();
            nal[0] = (uint8_t)(((rnd() % 48) << 1) | (rnd() & 0x81));
            const hbs::RtpNal u = hbs::rtp_nal(L, w.mp, 0);
            const uint32_t ts = (uint32_t)rnd();
            uint8_t* back = (uint8_t*)malloc(L);
            uint64_t got = 0, units, bytes;
            hbs::RtpuPacket prev;
            memset(&prev, 0, sizeof(prev));
            for (p = 0; p < u.packets; ++p, ++j) {
                cut = 0;
                const uint64_t plen = hbs::rtp_packet_bytes(w, L, u, p);
                uint8_t* out = (uint8_t*)malloc(plen);
                hbs::rtp_write_packet_host(w, nal, L, p, true, j, ts, out);
                const hbs::RtpuPacket r = read_exact(out, plen, q, &units, &bytes);
                CHECK(r.seq == ((65530 + j) & 0xFFFF) && r.ts == ts && r.ssrc == up.ssrc && r.pay_off == 12 && r.pay_len == plen - 12 && r.pad == 0);
                CHECK(r.marker == (p + 1 == u.packets ? 1u : 0u));
                if (!u.fu) {
                    CHECK(r.cls == hbs::kRtpuSingle && !hbs::rtpu_continues(r, prev));
                    memcpy(back, out + 12, L); got = L;
                } else {
                    CHECK(r.cls == hbs::kRtpuFu && r.fu_s == (p == 0 ? 1u : 0u) && r.fu_e == (p + 1 == u.packets ? 1u : 0u) && r.fu_type == ((nal[0] >> 1) & 63u));
                    CHECK(hbs::rtpu_continues(r, prev) == (p != 0));
                    if (p) {                                              /* what breaks a chain */
                        hbs::RtpuPacket x = r;
                        x.seq = (x.seq + 1) & 0xFFFF; CHECK(!hbs::rtpu_continues(x, prev)); x = r;
                        x.ts ^= 1; CHECK(!hbs::rtpu_continues(x, prev)); x = r;
                        x.h1 ^= 1; CHECK(!hbs::rtpu_continues(x, prev)); x = r;
                        x.fu_type ^= 1; CHECK(!hbs::rtpu_continues(x, prev)); x = r;
                        x.ssrc ^= 1; CHECK(!hbs::rtpu_continues(x, prev)); x = r;
                        x.fu_s = 1; CHECK(!hbs::rtpu_continues(x, prev));
                        hbs::RtpuPacket y = prev;
                        y.fu_e = 1; CHECK(!hbs::rtpu_continues(r, y)); y = prev;
                        y.cls = hbs::kRtpuOther; CHECK(!hbs::rtpu_continues(r, y));
                    }
                    if (p == 0) {
                        const uint64_t lit = hbs::rtpu_literal(4, true, r.h0, r.fu_type, r.h1);
                        back[0] = (uint8_t)(lit >> 32); back[1] = (uint8_t)(lit >> 40); got = 2;
                    }
                    CHECK(got + r.pay_len - 3 <= L);
                    memcpy(back + got, out + 15, r.pay_len - 3); got += r.pay_len - 3;
                }
                prev = r;
                /* another payload type, another ssrc: not this stream's */
                out[1] ^= 1; CHECK(read_exact(out, plen, q, &units, &bytes).cls == hbs::kRtpuOther); out[1] ^= 1;
                out[11] ^= 1; CHECK(read_exact(out, plen, q, &units, &bytes).cls == hbs::kRtpuOther); out[11] ^= 1;
                /* truncated by 1 .. all bytes: a fault, or a shorter valid packet of the same header */
                for (cut = 1; cut <= plen; ++cut) {
                    const hbs::RtpuPacket t = read_exact(out, plen - cut, q, &units, &bytes);
                    if (t.cls == hbs::kRtpuFault) { CHECK(plen - cut < 12 || (u.fu && plen - cut < 15)); ++faults; }
                    else { CHECK(plen - cut >= 12 && t.pay_len == plen - cut - 12 && t.seq == r.seq); ++shorter; }
                }
                free(out);
            }
            cut = 0;
            CHECK(got == L && memcmp(back, nal, L) == 0);
            free(back); free(nal);
        }
    }

    /* aggregation packets of 1 .. 8 units, with CSRC entries, an extension and padding in front of and behind some; cut short */
    for (int n_units = 1; n_units <= 8; ++n_units)
    for (int form = 0; form < 4; ++form) {
        L = (uint64_t)n_units; p = (uint64_t)form; cut = 0; mp = 0;
        uint8_t buf[600];
        uint64_t n = 12;
        memset(buf, 0, sizeof(buf));
        const uint32_t csrc = form & 1 ? 3u : 0u, ext_words = form & 2 ? 2u : 0u, pad = form == 3 ? 5u : 0u;
        buf[0] = (uint8_t)(0x80 | csrc | (form & 2 ? 0x10 : 0) | (pad ? 0x20 : 0)); buf[1] = 96;
        buf[8] = 0xCA; buf[9] = 0xFE; buf[10] = 0x00; buf[11] = 0x01;
        n += 4 * csrc;
        if (form & 2) { buf[n] = 0xBE; buf[n + 1] = 0xDE; buf[n + 2] = 0; buf[n + 3] = (uint8_t)ext_words; n += 4 + 4 * ext_words; }
        const uint64_t pay = n;
        buf[n++] = 48 << 1; buf[n++] = 1;
        uint64_t sizes[8], total = 0;
        for (int i = 0; i < n_units; ++i) {
            sizes[i] = 2 + rnd() % 40; total += sizes[i];
            buf[n++] = (uint8_t)(sizes[i] >> 8); buf[n++] = (uint8_t)sizes[i];
            buf[n] = (uint8_t)((rnd() % 48) << 1);
            for (uint64_t b = 1; b < sizes[i]; ++b) buf[n + b] = (uint8_t)rnd();
            n += sizes[i];
        }
        const uint64_t pay_len = n - pay;
        if (pad) { n += pad; buf[n - 1] = (uint8_t)pad; }
        uint64_t units, bytes;
        hbs::RtpuPacket r = read_exact(buf, n, q, &units, &bytes);
        CHECK(r.cls == hbs::kRtpuAp && units == (uint64_t)n_units && bytes == total && r.pay_off == pay && r.pay_len == pay_len && r.pad == pad);
        for (cut = 1; cut <= n; ++cut) {
            const hbs::RtpuPacket t = read_exact(buf, n - cut, q, &units, &bytes);
            if (t.cls == hbs::kRtpuFault) ++faults;
            else { CHECK((t.cls == hbs::kRtpuAp && units >= 1 && units <= (uint64_t)n_units) || (t.cls == hbs::kRtpuUnsupported && t.pay_len < 2)); ++shorter; }
        }
        cut = 0;
        /* each malformed form */
        uint8_t* at_size = buf + pay + 2;
        at_size[0] = 0xFF; at_size[1] = 0xFF; CHECK(read_exact(buf, n, q, &units, &bytes).cls == hbs::kRtpuFault);
        at_size[0] = 0; at_size[1] = (uint8_t)(pay_len - 4 + 1); CHECK(read_exact(buf, n, q, &units, &bytes).cls == hbs::kRtpuFault);
        at_size[1] = 1; CHECK(read_exact(buf, n, q, &units, &bytes).cls == hbs::kRtpuFault);
        at_size[1] = 0; CHECK(read_exact(buf, n, q, &units, &bytes).cls == hbs::kRtpuFault);
        at_size[1] = (uint8_t)sizes[0];
        at_size[2] = 48 << 1; CHECK(read_exact(buf, n, q, &units, &bytes).cls == hbs::kRtpuFault);
        at_size[2] = 63 << 1; CHECK(read_exact(buf, n, q, &units, &bytes).cls == hbs::kRtpuFault);
        at_size[2] = 47 << 1; CHECK(read_exact(buf, n, q, &units, &bytes).cls == hbs::kRtpuAp);
    }
    {   /* no unit, PACI, reserved types, a payload of one byte and of none, an FU of type 48 */
        uint8_t pkt[16] = {0x80, 96, 0, 1, 0, 0, 0, 2, 0xCA, 0xFE, 0x00, 0x01, 48 << 1, 1, 0, 0};
        uint64_t units, bytes;
        L = p = cut = 0; mp = 0;
        CHECK(read_exact(pkt, 14, q, &units, &bytes).cls == hbs::kRtpuFault);
        CHECK(read_exact(pkt, 15, q, &units, &bytes).cls == hbs::kRtpuFault);
        CHECK(read_exact(pkt, 13, q, &units, &bytes).cls == hbs::kRtpuUnsupported && read_exact(pkt, 12, q, &units, &bytes).cls == hbs::kRtpuUnsupported);
        for (int t = 50; t < 64; ++t) { pkt[12] = (uint8_t)(t << 1); CHECK(read_exact(pkt, 16, q, &units, &bytes).cls == hbs::kRtpuUnsupported); }
        pkt[12] = 49 << 1; pkt[14] = 0x80 | 48; CHECK(read_exact(pkt, 16, q, &units, &bytes).cls == hbs::kRtpuFault);
        pkt[14] = 0xC0 | 47; CHECK(read_exact(pkt, 16, q, &units, &bytes).cls == hbs::kRtpuFu && read_exact(pkt, 15, q, &units, &bytes).cls == hbs::kRtpuFu);
        CHECK(read_exact(pkt, 14, q, &units, &bytes).cls == hbs::kRtpuFault);
        CHECK(hbs::rtpu_accepted(hbs::kRtpuUnsupported) && hbs::rtpu_accepted(hbs::kRtpuFu) && !hbs::rtpu_accepted(hbs::kRtpuOther) && !hbs::rtpu_accepted(hbs::kRtpuFault));
    }

    /* hbs_rtp_frames_host: a framed stream in an exactly sized block, whole and cut short at every byte */
    {
        L = p = cut = 0; mp = 0;
        const uint64_t lens[] = {12, 0, 1, 300, 70, 2, 65535, 13};
        uint64_t n = 0;
        for (int i = 0; i < 8; ++i) n += 2 + lens[i];
        uint8_t* stream = (uint8_t*)malloc(n);
        uint64_t at = 0, begin[9];
        for (int i = 0; i < 8; ++i) {
            begin[i] = at;
            stream[at] = (uint8_t)(lens[i] >> 8); stream[at + 1] = (uint8_t)lens[i];
            for (uint64_t b = 0; b < lens[i]; ++b) stream[at + 2 + b] = (uint8_t)rnd();
            at += 2 + lens[i];
        }
        begin[8] = at;
        for (cut = 0; cut <= n; cut += (cut > 400 && cut + 700 < n ? 97 : 1)) {
            const uint64_t m = n - cut;
            uint8_t* part = (uint8_t*)malloc(m ? m : 1);
            memcpy(part, stream, m);
            uint64_t whole = 0;
            while (whole < 8 && begin[whole + 1] <= m) ++whole;
            for (uint64_t cap = 0; cap <= 9; cap += 3) {
                uint64_t* off = (uint64_t*)malloc(cap ? cap * 8 : 1);
                uint64_t* size = (uint64_t*)malloc(cap ? cap * 8 : 1);
                uint64_t used = ~0ull;
                CHECK(hbs::rtp_frames_host(part, m, off, size, cap, &used) == whole && used == begin[whole]);
                for (uint64_t i = 0; i < whole && i < cap; ++i) CHECK(off[i] == begin[i] + 2 && size[i] == lens[i] && off[i] + size[i] <= m);
                free(off); free(size);
            }
            CHECK(hbs::rtp_frames_host(part, m, nullptr, nullptr, 4, nullptr) == whole);
            free(part);
        }
        cut = 0;
        uint64_t used = 5;
        CHECK(hbs::rtp_frames_host(nullptr, 100, nullptr, nullptr, 0, &used) == 0 && used == 0);
        free(stream);
    }
    printf("%lu packets read, %lu truncated packets refused, %lu read as shorter packets\n", reads, faults, shorter);
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
    src = tmp_path / "rtp_unpack_host_asan.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "rtp_unpack_host_asan"
    cmd = [cxx] + flags + ["-I", os.path.join(ROOT, "hevcbitstream_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "truncated packets refused" in run.stdout
