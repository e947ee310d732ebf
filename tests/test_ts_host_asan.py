"""The host entry points of hbs_ts.h under AddressSanitizer and UBSan, in a stand-alone program: both functions over exactly
sized heap blocks of every length 0..2 B + 1, random and with hostile length bytes.  Nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "hbs_ts.h"

static uint64_t state = 0x1234567ull;
static uint32_t rnd() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(state >> 33); }

/* a packet head that leads the walk as far as it can go: a PAT / PMT with hostile lengths */
static void plant(uint8_t* b, uint64_t n, int B, int kind)
{
    const uint64_t h = B == 192 ? 4 : 0;
    for (uint64_t p = 0; (p + 1) * B <= n; ++p) {
        uint8_t* t = b + p * B + h;
        const int pid = (p & 1) ? 0x1000 : 0;
        t[0] = 0x47; t[1] = 0x40 | (pid >> 8); t[2] = pid & 0xFF; t[3] = (kind & 1) ? 0x30 : 0x10;
        uint32_t at = 4;
        if (kind & 1) { t[4] = (uint8_t)(rnd() % 186); at = 5 + t[4]; }
        if (at >= 188) continue;
        t[at] = (kind & 2) ? (uint8_t)rnd() : (uint8_t)(rnd() % 4);                    /* pointer_field */
        uint32_t s = at + 1 + t[at];
        if (s + 3 > 188) continue;
        t[s] = pid ? 2 : 0;
        const uint32_t len = (kind & 4) ? (rnd() & 0xFFF) : (188 - s - 3 - (rnd() % 3));
        t[s + 1] = 0xB0 | (len >> 8); t[s + 2] = len & 0xFF;
        if (!pid && s + 12 <= 188) { t[s + 8] = 0; t[s + 9] = 1; t[s + 10] = 0xF0; t[s + 11] = 0x00; }
        if (pid && s + 12 <= 188) {
            t[s + 10] = 0xF0 | (rnd() & 15 & ((kind & 8) ? 15 : 0)); t[s + 11] = (uint8_t)(rnd() % ((kind & 8) ? 256 : 8));
            const uint32_t es = s + 12 + (((t[s + 10] & 15u) << 8) | t[s + 11]);
            if (es + 5 <= 188) { t[es] = 0x24; t[es + 1] = 0xE1; t[es + 2] = 0x00; t[es + 3] = 0xF0; t[es + 4] = (kind & 2) ? 0xFF : 0; }
        }
    }
}

int main()
{
    unsigned long calls = 0, found = 0;
    const int sizes[3] = {188, 192, 204};
    for (int si = 0; si < 3; ++si) {
        const int B = sizes[si];
        for (uint64_t n = 0; n <= 2 * (uint64_t)B + 1; ++n) {
            for (int kind = 0; kind < 24; ++kind) {
                uint8_t* b = (uint8_t*)malloc(n ? n : 1);              /* exactly n bytes are valid */
                if (n == 0) { free(b); b = nullptr; }
                for (uint64_t i = 0; i < n; ++i) b[i] = (kind >= 16 && (rnd() & 3)) ? 0xFF : (uint8_t)rnd();
                if (kind < 16) plant(b, n, B, kind);
                int prog = -1;
                const int pid = hbs::ts_find_pid_host(b, n, B, kind < 16 ? 0x24 : b ? b[n / 2] : 0, &prog);
                if (pid >= 0) ++found;
                if (pid < -1 || pid > 8191) { fprintf(stderr, "pid %d\n", pid); return 2; }
                ++calls;
                for (uint64_t p = 0; (p + 1) * B <= n; ++p) {
                    /* the packet alone in a block of its own: a read behind it is a read behind the block */
                    uint8_t* one = (uint8_t*)malloc(B);
                    memcpy(one, b + p * B, B);
                    const uint64_t h = B == 192 ? 4 : 0;
                    if (kind & 1) one[h] = 0x47;
                    if (kind & 2) { one[h + 1] = 0x41; one[h + 2] = 0x00; }
                    if (kind & 4) one[h + 3] = (uint8_t)((one[h + 3] & 0x0F) | 0x30), one[h + 4] = (uint8_t)(160 + rnd() % 96);
                    hbs_ts_packet r;
                    if (hbs::ts_packet_host(one, B, 0x100, &r) != 0) return 3;
                    if (r.cls >= HBS_TS_PAYLOAD && (r.off + r.len != 188 || r.es_off + r.es_len != 188 || r.es_off < r.off)) return 4;
                    free(one);
                    ++calls;
                }
                free(b);
            }
        }
    }
    if (!found) { fprintf(stderr, "the planted tables were never followed to a PID\n"); return 5; }
    printf("%lu calls, %lu PIDs found\n", calls, found);
    return 0;
}
"""


def test_host_functions_under_sanitizers(tmp_path):
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
    src = tmp_path / "ts_host_asan.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "ts_host_asan"
    cmd = [cxx] + flags + ["-I", os.path.join(ROOT, "hevcbitstream_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "PIDs found" in run.stdout
