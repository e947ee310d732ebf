"""The rules of hbs_cbcs.h (cbcs_expand_dec_key, cbcs_aes_inv_block, cbcs_pattern, cbcs_is_crypt, cbcs_crypt_blocks, cbcs_block_of,
cbcs_params_ok) and the forward cipher of hbs_cenc.h under AddressSanitizer and UBSan, in a stand-alone program: both key
schedules, both block functions, predicate and count, what the call refuses, and the walk of hbs_cbcs.hip single-stepped on the
host -- entry by entry as a lane goes, and in steps of 64 crypt blocks as a decrypting wavefront goes, all of a step's loads in
front of its stores -- over tables and data in exactly sized heap blocks.  The program prints counts and digests;
tests/_cbcs_ref.py must say the same of every case.  Nothing is loaded into python."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import _cbcs_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "hevcbitstream_amd.h"
#include "hbs_cbcs.h"

using namespace hbs;

static uint64_t digest(const uint8_t* p, uint64_t n)
{
    uint64_t h = 0;
    for (uint64_t i = 0; i < n; ++i) h = h * 1099511628211ull + p[i];
    return h;
}

template <class T> static T* block(FILE* f, uint64_t n)        /* a heap block of exactly n records, read from the file */
{
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    if (n && fread(p, sizeof(T), n, f) != n) exit(4);
    return p;
}

static void store_be(const uint32_t w[4], uint8_t* b)
{
    for (int i = 0; i < 16; ++i) b[i] = (uint8_t)(w[i >> 2] >> (24 - 8 * (i & 3)));
}
static uint64_t key_digest(const CencKey& k)
{
    uint8_t b[176];
    for (int r = 0; r < 11; ++r) store_be(k.rk + 4 * r, b + 16 * r);
    return digest(b, 176);
}
static void enc(const CencKey& k, const uint32_t in[4], uint32_t out[4]) { cenc_aes_block(k, in, out, [](uint32_t x) { return cenc_te0(x); }); }
static void dec(const CencKey& k, const uint32_t in[4], uint32_t out[4])
{
    cbcs_aes_inv_block(k, in, out, [](uint32_t x) { return cbcs_td0_of(cbcs_inv_sbox(x)); }, [](uint32_t x) { return cbcs_inv_sbox(x); });
}

static void key_case(FILE* f)
{
    uint8_t key[16];
    if (fread(key, 16, 1, f) != 1) exit(4);
    CencKey ek, dk;
    cenc_expand_key(key, ek);
    cbcs_expand_dec_key(ek, dk);
    printf("key %llu %llu\n", (unsigned long long)key_digest(ek), (unsigned long long)key_digest(dk));
}

static void block_case(FILE* f)
{
    uint8_t key[16];
    uint64_t n;
    if (fread(key, 16, 1, f) != 1 || fread(&n, 8, 1, f) != 1) exit(4);
    uint8_t* in = block<uint8_t>(f, n * 16);
    uint8_t* e = (uint8_t*)malloc(n ? n * 16 : 1);
    uint8_t* d = (uint8_t*)malloc(n ? n * 16 : 1);
    CencKey ek, dk;
    cenc_expand_key(key, ek);
    cbcs_expand_dec_key(ek, dk);
    for (uint64_t j = 0; j < n; ++j) {
        uint32_t x[4], y[4], z[4];
        cbcs_load_be(in + 16 * j, x);
        enc(ek, x, y); store_be(y, e + 16 * j);
        dec(dk, x, z); store_be(z, d + 16 * j);
        dec(dk, y, z);
        if (memcmp(z, x, 16) != 0) exit(6);
    }
    printf("blocks %llu %llu\n", (unsigned long long)digest(e, n * 16), (unsigned long long)digest(d, n * 16));
    free(in); free(e); free(d);
}

static void pattern_case()
{
    std::vector<uint8_t> counts;
    for (uint32_t c = 0; c < 16; ++c) for (uint32_t k = 0; k < 16; ++k) {
        if (c == 0 && k != 0) continue;
        for (uint32_t flags = 0; flags <= HBS_CBCS_WHOLE_RUNS; flags += HBS_CBCS_WHOLE_RUNS) {
            const CbcsPattern p = cbcs_pattern(c, k, flags);
            for (uint32_t nb = 0; nb <= 70; ++nb) {
                uint32_t n = 0;
                for (uint32_t i = 0; i < nb + 40; ++i) if (cbcs_is_crypt(p, nb, i)) { if (i >= nb || cbcs_block_of(p, n) != i) exit(7); n += 1; }
                if (n != cbcs_crypt_blocks(p, nb)) exit(8);
                counts.push_back((uint8_t)n);
            }
        }
    }
    printf("pattern %llu %llu\n", (unsigned long long)counts.size(), (unsigned long long)digest(counts.data(), counts.size()));
}

static void params_case(FILE* f)
{
    uint64_t n;
    if (fread(&n, 8, 1, f) != 1) exit(4);
    hbs_cbcs_params* p = block<hbs_cbcs_params>(f, n);
    printf("params %d", cbcs_params_ok(nullptr) ? 1 : 0);
    for (uint64_t i = 0; i < n; ++i) printf("%d", cbcs_params_ok(p + i) ? 1 : 0);
    printf("\n");
    free(p);
}

static void crypt_case(FILE* f)
{
    hbs_cbcs_params prm;
    uint64_t hd[3];          /* data bytes, samples, entries in the table */
    if (fread(&prm, 48, 1, f) != 1 || fread(hd, 8, 3, f) != 3) exit(4);
    const uint64_t n = hd[0], ns = hd[1];
    uint8_t* data = block<uint8_t>(f, n);
    uint64_t* off = block<uint64_t>(f, ns);
    uint64_t* size = block<uint64_t>(f, ns);
    uint64_t* first = block<uint64_t>(f, ns + 1);
    hbs_cenc_subsample* sub = block<hbs_cenc_subsample>(f, hd[2]);
    uint8_t* iv = block<uint8_t>(f, ns * 16);
    if (!cbcs_params_ok(&prm)) { printf("refused\n"); free(data); free(off); free(size); free(first); free(sub); free(iv); return; }
    const CbcsPattern pat = cbcs_pattern(prm.crypt_byte_block, prm.skip_byte_block, prm.flags);
    const bool decrypt = (prm.flags & HBS_CBCS_DECRYPT) != 0;
    CencKey ek, dk;
    cenc_expand_key(prm.key, ek);
    cbcs_expand_dec_key(ek, dk);
    uint64_t bad = 0, total = 0;
    for (uint64_t s = 0; s < ns && !bad; ++s)
        if (!cenc_sample_ok(s, off[s], size[s], s + 1 < ns, s + 1 < ns ? off[s + 1] : 0, n, first[s], first[s + 1])) bad = s + 1;
    for (uint64_t s = 0; s < ns && !bad; ++s) {
        uint64_t sum = 0;
        for (uint64_t e = first[s]; e < first[s + 1]; ++e) { sum += (uint64_t)sub[e].clear + sub[e].protect; if (sub[e].clear > kCencMaxClear) bad = s + 1; }
        if (sum != size[s]) bad = s + 1;
    }
    if (bad) { printf("arg %llu\n", (unsigned long long)bad); goto done; }
    for (uint64_t s = 0; s < ns; ++s) {
        uint32_t ivw[4];
        cbcs_load_be(prm.iv_mode ? prm.iv0 : iv + 16 * s, ivw);
        uint64_t p = off[s];
        for (uint64_t e = first[s]; e < first[s + 1]; ++e) {
            p += sub[e].clear;
            const uint32_t cnt = cbcs_crypt_blocks(pat, sub[e].protect >> 4);
            total += cnt;
            if (decrypt && cnt >= kCbcsLaneBlocks) {
                /* a wavefront: 64 crypt blocks a step, every load of the step in front of its stores */
                uint32_t carry[4] = {ivw[0], ivw[1], ivw[2], ivw[3]};
                for (uint32_t base = 0; base < cnt; base += 64) {
                    uint32_t x[64][4];
                    const uint32_t lanes = cnt - base < 64 ? cnt - base : 64;
                    for (uint32_t l = 0; l < lanes; ++l) cbcs_load_be(data + p + 16ull * cbcs_block_of(pat, base + l), x[l]);
                    for (uint32_t l = 0; l < lanes; ++l) {
                        uint32_t y[4];
                        const uint32_t* prev = l ? x[l - 1] : carry;
                        dec(dk, x[l], y);
                        for (int i = 0; i < 4; ++i) y[i] ^= prev[i];
                        store_be(y, data + p + 16ull * cbcs_block_of(pat, base + l));
                    }
                    if (lanes == 64) memcpy(carry, x[63], 16);
                }
            } else {
                /* a lane: block by block, the previous ciphertext in registers */
                uint32_t prev[4] = {ivw[0], ivw[1], ivw[2], ivw[3]};
                uint64_t q = p;
                uint32_t r = 0;
                for (uint32_t j = 0; j < cnt; ++j) {
                    uint32_t x[4], y[4];
                    cbcs_load_be(data + q, x);
                    if (decrypt) { dec(dk, x, y); for (int i = 0; i < 4; ++i) { y[i] ^= prev[i]; prev[i] = x[i]; } }
                    else { for (int i = 0; i < 4; ++i) x[i] ^= prev[i]; enc(ek, x, y); memcpy(prev, y, 16); }
                    store_be(y, data + q);
                    q += 16; r += 1;
                    if (r == pat.c) { r = 0; q += 16u * pat.k; }
                }
            }
            p += sub[e].protect;
        }
    }
    printf("ok %llu %llu %llu\n", (unsigned long long)first[ns], (unsigned long long)(16 * total), (unsigned long long)digest(data, n));
done:
    free(data); free(off); free(size); free(first); free(sub); free(iv);
}

int main(int argc, char** argv)
{
    static_assert(sizeof(hbs_cbcs_params) == 48 && sizeof(hbs_cenc_subsample) == 8, "layouts");
    FILE* f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    if (!f) return 3;
    for (;;) {
        const int kind = fgetc(f);
        if (kind == EOF) break;
        if (kind == 'K') key_case(f);
        else if (kind == 'B') block_case(f);
        else if (kind == 'P') pattern_case();
        else if (kind == 'O') params_case(f);
        else if (kind == 'C') crypt_case(f);
        else return 5;
    }
    fclose(f);
    return 0;
}
"""

H = bytes.fromhex
KEY_197, KEY_38A = bytes(range(16)), H("2b7e151628aed2a6abf7158809cf4f3c")
PLAIN_38A = H("6bc1bee22e409f96e93d7e117393172a" "ae2d8a571e03ac9c9eb76fac45af8e51" "30c81c46a35ce411e5fbc1191a0a52ef" "f69f2445df4f9b17ad2b417be66c3710")
CBC_38A = H("7649abac8119b246cee98e9b12e9197d" "5086cb9b507219ee95db113a917678b2" "73bed6b8e3c1743b7116e69e22229516" "3ff1caa1681fac09120eca307586e1a7")


def digest(raw):
    h = 0
    for v in bytes(raw):
        h = (h * 1099511628211 + v) & ((1 << 64) - 1)
    return h


def dec_schedule(key):
    """the round keys of the equivalent inverse cipher (FIPS-197 5.3.5): reversed, InvMixColumns on rounds 1..9"""
    out = []
    for r, k in enumerate(reversed(R.expand_key(key))):
        if 0 < r < 10:
            k = bytes(R._gmul(k[4 * c + i], 14) ^ R._gmul(k[4 * c + (i + 1) % 4], 11) ^ R._gmul(k[4 * c + (i + 2) % 4], 13) ^ R._gmul(k[4 * c + (i + 3) % 4], 9)
                      for c in range(4) for i in range(4))
        out.append(k)
    return b"".join(out)


def params_rows():
    rows = []
    for iv_mode, flags, c, k, r0, r1 in ((0, 0, 1, 9, 0, 0), (1, 3, 0, 0, 0, 0), (2, 0, 1, 9, 0, 0), (0, 4, 1, 9, 0, 0), (0, 0, 16, 0, 0, 0), (0, 0, 1, 16, 0, 0),
                                        (0, 0, 0, 1, 0, 0), (0, 0, 15, 15, 0, 0), (0, 0, 1, 9, 1, 0), (0, 0, 1, 9, 0, 1), (1, 1, 3, 7, 0, 0), (0, 0x80000000, 1, 9, 0, 0)):
        p = np.zeros(1, dtype=R.PARAMS)
        p["iv_mode"], p["flags"], p["crypt_byte_block"], p["skip_byte_block"], p["reserved0"], p["reserved1"] = iv_mode, flags, c, k, r0, r1
        rows.append((p.tobytes(), R.params_ok(iv_mode, flags, c, k, r0, r1)))
    return rows


def make_entries(rng, n_samples, extra=()):
    """samples of 0..5 random entries with random gaps, then one sample for each list of `extra`: (data_bytes, off, size, first, sub)"""
    subs, first, off, size, at = [], [0], [], [], int(rng.integers(0, 40))
    for s in range(n_samples + len(extra)):
        if s < n_samples:
            e = [(int(rng.integers(0, 60)) if rng.integers(0, 3) else 0, int(rng.integers(0, 520)) if rng.integers(0, 5) else 0)
                 for _ in range(int(rng.integers(0, 6)))]
        else:
            e = list(extra[s - n_samples])
        subs += e
        first.append(len(subs))
        off.append(at)
        size.append(sum(a + b for a, b in e))
        at += size[-1] + int(rng.integers(0, 30))
    return (at, np.array(off, dtype=np.uint64), np.array(size, dtype=np.uint64), np.array(first, dtype=np.uint64),
            np.array(subs, dtype=R.SUBSAMPLE).reshape(-1))


def crypt_cases():
    rng = np.random.default_rng(2402)
    out = []
    long = [[(3, 16 * 63 + 5)], [(0, 16 * 64)], [(7, 16 * 65 + 15), (2, 16 * 130)]]          # around the lane / wavefront threshold at 1:0
    for n_samples, extra, mode, c, k, flags in ((0, (), 1, 1, 9, 0), (150, (), 0, 1, 9, 0), (150, (), 0, 1, 9, 1), (80, long, 1, 1, 0, 0), (80, long, 1, 0, 0, 1),
                                                (120, (), 0, 3, 7, 0), (120, (), 1, 3, 7, 3), (60, ([(1, 16 * 700 + 3)],), 0, 1, 9, 1), (90, (), 1, 2, 1, 2),
                                                (90, long, 0, 15, 15, 1), (5, (), 0, 0, 3, 0)):
        n, off, size, first, sub = make_entries(rng, n_samples, extra)
        out.append(dict(n=n, off=off, size=size, first=first, sub=sub, mode=mode, c=c, k=k, flags=flags, data=rng.integers(0, 256, n, dtype=np.uint8),
                        key=bytes(rng.integers(0, 256, 16, dtype=np.uint8)), iv0=bytes(rng.integers(0, 256, 16, dtype=np.uint8)),
                        iv=rng.integers(0, 256, 16 * len(off), dtype=np.uint8)))
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in out[1].items()}
    bad["size"][11] += 1
    out.append(bad)
    return out


def crypt_record(c):
    prm = np.zeros(1, dtype=R.PARAMS)
    prm["key"][0] = np.frombuffer(c["key"], dtype=np.uint8)
    prm["iv0"][0] = np.frombuffer(c["iv0"], dtype=np.uint8)
    prm["iv_mode"], prm["flags"], prm["crypt_byte_block"], prm["skip_byte_block"] = c["mode"], c["flags"], c["c"], c["k"]
    return (b"C" + prm.tobytes() + struct.pack("<3Q", c["n"], len(c["off"]), len(c["sub"])) + c["data"].tobytes() + c["off"].tobytes() +
            c["size"].tobytes() + c["first"].tobytes() + c["sub"].tobytes() + c["iv"].tobytes())


def crypt_want(c):
    if not R.params_ok(c["mode"], c["flags"], c["c"], c["k"]):
        return "refused"
    bad = R.crypt_check(c["n"], c["off"], c["size"], c["first"], c["sub"])
    if bad:
        return "arg %d" % bad
    data, done = R.crypt_many(c["data"], c["off"], c["size"], c["first"], c["sub"], c["key"], iv=c["iv"] if c["mode"] == 0 else None,
                              iv0=c["iv0"] if c["mode"] else None, c=c["c"], k=c["k"], whole=bool(c["flags"] & R.WHOLE_RUNS),
                              decrypt=bool(c["flags"] & R.DECRYPT))
    return "ok %d %d %d" % (len(c["sub"]), done, digest(data.tobytes()))


def test_rules_single_stepped_under_sanitizers(tmp_path):
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
    src = tmp_path / "cbcs_host_asan.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "cbcs_host_asan"
    cmd = [cxx] + flags + ["-I", os.path.join(ROOT, "hevcbitstream_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    rng = np.random.default_rng(2403)
    want = []
    with open(tmp_path / "cases.bin", "wb") as f:
        for key in (KEY_197, KEY_38A, bytes(16), bytes(rng.integers(0, 256, 16, dtype=np.uint8))):
            f.write(b"K" + key)
            want.append("key %d %d" % (digest(b"".join(R.expand_key(key))), digest(dec_schedule(key))))
        for key, blocks in ((KEY_197, H("00112233445566778899aabbccddeeff") + H("69c4e0d86a7b0430d8cdb78070b4c55a")), (KEY_38A, PLAIN_38A + CBC_38A),
                            (bytes(rng.integers(0, 256, 16, dtype=np.uint8)), rng.integers(0, 256, 16 * 50, dtype=np.uint8).tobytes()), (bytes(16), b"")):
            f.write(b"B" + key + struct.pack("<Q", len(blocks) // 16) + blocks)
            arr = np.frombuffer(blocks, dtype=np.uint8).reshape(-1, 16)
            want.append("blocks %d %d" % (digest(R.encrypt_blocks(key, arr).tobytes()), digest(R.decrypt_blocks(key, arr).tobytes())))
        f.write(b"P")
        counts = bytes(R.crypt_blocks(c, k, whole, nb) for c in range(16) for k in range(16) if not (c == 0 and k) for whole in (False, True)
                       for nb in range(71))
        want.append("pattern %d %d" % (len(counts), digest(counts)))
        rows = params_rows()
        f.write(b"O" + struct.pack("<Q", len(rows)) + b"".join(r for r, _ in rows))
        want.append("params 0" + "".join("1" if ok else "0" for _, ok in rows))
        for c in crypt_cases():
            f.write(crypt_record(c))
            want.append(crypt_want(c))
    run = subprocess.run([str(exe), str(tmp_path / "cases.bin")], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-6000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(want)
    for i, (got, exp) in enumerate(zip(lines, want)):
        assert got == exp, i
    assert {ln.split()[0] for ln in lines} == {"key", "blocks", "pattern", "params", "ok", "arg", "refused"}
    # the published answers themselves: FIPS-197 C.1 both ways, and the CBC vector through the two block functions
    assert bytes(R.encrypt_blocks(KEY_197, np.frombuffer(H("00112233445566778899aabbccddeeff"), dtype=np.uint8))[0]).hex() == "69c4e0d86a7b0430d8cdb78070b4c55a"
    assert bytes(R.decrypt_blocks(KEY_197, np.frombuffer(H("69c4e0d86a7b0430d8cdb78070b4c55a"), dtype=np.uint8))[0]).hex() == "00112233445566778899aabbccddeeff"
    assert R.cbc(KEY_38A, bytes(range(16)), PLAIN_38A) == CBC_38A
