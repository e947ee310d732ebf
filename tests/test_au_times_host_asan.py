"""The rules of hbs_autimes.h (aut_params_ok, aut_ukey, aut_seg_combine, aut_seg_value, aut_rank with its two steps, aut_dts,
aut_pts, aut_late, aut_lag) under AddressSanitizer and UBSan, in a stand-alone program: the plan of hbs_autimes.hip single-stepped
on the host -- digest, the three scans over workgroups of kAutLanes AUs, apply, the walk, reduce, write -- over AU tables and
scratch in exactly sized heap blocks.  The program prints the summary and a digest of each output table; tests/_au_times_ref.py
must say the same of every case.  Nothing is loaded into python."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import _au_times_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "hevcbitstream_amd.h"
#include "hbs_autimes.h"

using namespace hbs;

static uint64_t digest(const std::vector<uint64_t>& v)
{
    uint64_t h = 0;
    for (uint64_t x : v) h = h * 1099511628211ull + x;
    return h;
}

/* hbs_au_times on the host, workgroup by workgroup as the kernels go */
static void plan(const hbs_access_unit* au, uint64_t n, const hbs_au_times_params& prm)
{
    if (!aut_params_ok(&prm, n)) { printf("refused\n"); return; }
    const uint64_t blocks = aut_blocks(n);
    std::vector<uint32_t> key(n), pmax(n), smin(n), ord(n), part(blocks * 8);
    std::vector<uint8_t> bits(n);
    /* k_aut_digest */
    for (uint64_t blk = 0; blk < blocks; ++blk) {
        const uint64_t base = blk * kAutLanes;
        AutSeg last = aut_seg(0, 0), mx = aut_seg(0, 0), mn = aut_seg(0, 0);
        bool known_head = false, blind_head = false;
        uint32_t heads = 0, last_head = 0;
        for (int t = 0; t < kAutLanes && base + t < n; ++t) {
            const uint64_t k = base + t;
            const bool head = aut_is_head(k, au[k].flags), pic = aut_has_picture(au[k].flags);
            last = aut_seg_combine(last, aut_seg(pic ? 1u : 0u, pic ? aut_ukey(au[k].pic_order_cnt) : 0u));
            key[k] = last.f ? last.x : 0u;
            bits[k] = (uint8_t)((head ? kAutHead : 0u) | (pic ? kAutPic : 0u) | (last.f ? kAutKnown : 0u));
            mx = aut_seg_combine(mx, aut_seg(head ? 1u : 0u, key[k]));
            if (head) { (last.f ? known_head : blind_head) = true; heads += 1; last_head = (uint32_t)k + 1u; }
        }
        for (int e = kAutLanes - 1; e >= 0; --e) {
            const uint64_t k = base + e;
            if (k >= n) continue;
            const bool end = k + 1 == n || (e + 1 < kAutLanes ? (bits[k + 1] & kAutHead) != 0 : aut_is_head(k + 1, au[k + 1].flags));
            mn = aut_seg_combine(mn, aut_seg(end ? 1u : 0u, (bits[k] & kAutKnown) ? ~key[k] : 0u));
        }
        uint32_t* p = &part[blk * 8];
        p[kAutPKey] = last.x; p[kAutPMax] = mx.x; p[kAutPMin] = mn.x;
        p[kAutPBits] = (last.f ? kAutBPic : 0u) | (mx.f ? kAutBHead : 0u) | (mn.f ? kAutBEnd : 0u) | ((blind_head && !known_head) ? kAutBLead : 0u);
        p[kAutPHeads] = heads; p[kAutPLast] = last_head; p[kAutPLag] = 0; p[kAutPBad] = 0;
    }
    /* k_aut_parts */
    uint64_t segs = 0, last_head = 0;
    {
        AutSeg run = aut_seg(0, 0);
        for (uint64_t i = 0; i < blocks; ++i) {
            uint32_t* p = &part[i * 8];
            const AutSeg el = aut_seg((p[kAutPBits] & kAutBPic) ? 1u : 0u, p[kAutPKey]);
            p[kAutPKey] = run.x; run = aut_seg_combine(run, el);
            if ((p[kAutPBits] & kAutBLead) && p[kAutPKey] > p[kAutPMax]) p[kAutPMax] = p[kAutPKey];
            segs += p[kAutPHeads];
            if (p[kAutPLast] > last_head) last_head = p[kAutPLast];
        }
        run = aut_seg(0, 0);
        for (uint64_t i = 0; i < blocks; ++i) {
            uint32_t* p = &part[i * 8];
            const AutSeg el = aut_seg((p[kAutPBits] & kAutBHead) ? 1u : 0u, p[kAutPMax]);
            p[kAutPMax] = run.x; run = aut_seg_combine(run, el);
        }
        run = aut_seg(0, 0);
        for (uint64_t i = blocks; i-- > 0;) {
            uint32_t* p = &part[i * 8];
            const AutSeg el = aut_seg((p[kAutPBits] & kAutBEnd) ? 1u : 0u, p[kAutPMin]);
            p[kAutPMin] = run.x; run = aut_seg_combine(run, el);
        }
    }
    /* k_aut_apply */
    for (uint64_t blk = 0; blk < blocks; ++blk) {
        const uint64_t base = blk * kAutLanes;
        const uint32_t* p = &part[blk * 8];
        AutSeg inc = aut_seg(0, 0);
        for (int t = 0; t < kAutLanes && base + t < n; ++t) {
            const uint64_t k = base + t;
            if (!(bits[k] & kAutKnown)) key[k] = p[kAutPKey];
            inc = aut_seg_combine(inc, aut_seg(bits[k] & kAutHead, key[k]));
            pmax[k] = aut_seg_value(p[kAutPMax], inc);
        }
        inc = aut_seg(0, 0);
        for (int e = kAutLanes - 1; e >= 0; --e) {
            const uint64_t k = base + e;
            if (k >= n) continue;
            const bool end = k + 1 == n || (bits[k + 1] & kAutHead) != 0;
            inc = aut_seg_combine(inc, aut_seg(end ? 1u : 0u, ~key[k]));
            smin[k] = ~aut_seg_value(p[kAutPMin], inc);
        }
    }
    /* k_aut_rank, k_aut_reduce */
    const bool given = (prm.flags & HBS_AUT_DELAY_GIVEN) != 0;
    uint64_t R = 0, bad = 0, late = 0;
    for (uint64_t k = 0; k < n; ++k) {
        const AutRank r = aut_rank(k, n, [&](uint64_t b) {
            AutRec x;
            x.key = key[b]; x.pmax = pmax[b]; x.smin = smin[b]; x.head = bits[b] & kAutHead;
            return x;
        });
        ord[k] = r.order;
        if (r.bad) { if (!bad) bad = k + 1; continue; }
        if (aut_lag(k, r.order) > R) R = aut_lag(k, r.order);
        if (given && aut_late(k, r.order, prm.delay)) late += 1;
    }
    if (bad) { printf("depth %llu\n", (unsigned long long)bad); return; }
    const uint64_t delay = given ? prm.delay : R;
    /* k_aut_write */
    std::vector<uint64_t> dts(n), pts(n), order(n), display(n);
    for (uint64_t k = 0; k < n; ++k) {
        dts[k] = aut_dts(prm.base_time, prm.tick, k, prm.flags);
        pts[k] = aut_pts(prm.base_time, prm.tick, ord[k], delay, prm.flags);
        order[k] = ord[k]; display[ord[k]] = k;
    }
    printf("ok %llu %llu %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)n, (unsigned long long)segs,
           (unsigned long long)(n ? last_head - 1 : 0), (unsigned long long)delay, (unsigned long long)R, (unsigned long long)late,
           (unsigned long long)digest(dts), (unsigned long long)digest(pts), (unsigned long long)(digest(order) ^ (digest(display) << 1)));
}

int main(int argc, char** argv)
{
    static_assert(sizeof(hbs_au_times_params) == 32 && sizeof(hbs_access_unit) == 64, "layouts");
    FILE* f = argc > 1 ? fopen(argv[1], "rb") : nullptr;
    if (!f) return 3;
    for (;;) {
        hbs_au_times_params prm;
        uint64_t n;
        if (fread(&prm, 32, 1, f) != 1 || fread(&n, 8, 1, f) != 1) break;
        hbs_access_unit* au = (hbs_access_unit*)malloc(n ? n * 64 : 1);       /* a heap block of exactly n records */
        if (n && fread(au, 64, n, f) != n) return 4;
        plan(au, n, prm);
        free(au);
    }
    fclose(f);
    return 0;
}
"""


def digest(values):
    h = 0
    for v in values:
        h = (h * 1099511628211 + int(v)) & ((1 << 64) - 1)
    return h


def want(au, kw):
    if T.refused(len(au), **kw):
        return "refused"
    r = T.au_times(au, **kw)
    s = r["summary"]
    if s["error"]:
        return "depth %d" % s["reserved"][0]
    return "ok %d %d %d %d %d %d %d %d %d" % (s["nal_count"], s["nal_found"], s["rbsp_bytes"], s["reserved"][0], s["reserved"][1], s["reserved"][2],
                                              digest(r["dts"]), digest(r["pts"]),
                                              digest(r["order"]) ^ ((digest(r["display"]) << 1) & ((1 << 64) - 1)))


def cases():
    """[(AU table, params as keywords)]"""
    B = 256
    rng = np.random.default_rng(2207)
    out = [(T.table([]), {}), (T.table([]), dict(delay=7)), (T.table([5]), {}), (T.table([0, 3, 1, 2]), dict(tick=3003, base_time=900))]
    for n in (2, 63, 64, 65, B - 1, B, B + 1, 2 * B + 1):
        out.append((T.table(T.pyramid(8, n)[:n], junk=rng), dict(tick=2)))
    # heads on the edges of a workgroup, every AU a head, one segment over three workgroups
    p = T.pyramid(16, 50)
    out += [(T.table(p[:3 * B], heads=h), {}) for h in ([B - 1], [B], [B - 1, B], [63, 64], list(range(3 * B)), [])]
    # a head without a picture as a workgroup's last head, pictures only behind it; AUs without a picture everywhere
    for heads, nopic in (([B + 2], range(B, B + 5)), ([B], [B]), ([B, B + 3], range(B - 2, B + 4)), ([2 * B + 1], range(B + 1, 3 * B)),
                         ([], range(0, 3)), ([], range(0, B + 7)), ([5], range(3 * B - 9, 3 * B)), ([B + 9], range(B - 3, B + 9))):
        keys = rng.integers(-50, 50, 3 * B).tolist()
        keys = sorted(keys[:B]) + sorted(keys[B:])
        out.append((T.table(keys, heads=heads, nopic=nopic, junk=rng), {}))
    # the span limit, backwards and forwards, inside one segment over several workgroups
    for span in (T.MAX_SPAN, T.MAX_SPAN + 1):
        out.append((T.table([0] * 10 + [9] + [1] * (span - 1) + [2] + [50] * 40), {}))       # the 9 moves `span` slots back
        out.append((T.table([0] * 10 + [3] * span + [1] + [5] * 40), {}))                   # the 1 moves `span` slots forward
        out.append((T.table([3] * 300 + [7] + [5] * span + [9] * 5, heads=[200]), {}))
    # extreme keys, ties, delays, the wrap, the time limit
    lo, hi = -(1 << 31), (1 << 31) - 1
    out.append((T.table([hi, lo, hi, lo, 0, -1, 1, hi, lo]), dict(base_time=(1 << 33) - 5, tick=3, flags=T.WRAP33)))
    g8 = T.pyramid(8, 6)
    out += [(T.table(g8), dict(delay=d, tick=3003)) for d in (0, 2, 3, 4, 1000)]
    out.append((T.table(g8), dict(base_time=T.LIMIT - 1 - (len(g8) + T.MAX_SPAN))))
    out.append((T.table(g8), dict(base_time=T.LIMIT - (len(g8) + T.MAX_SPAN))))
    out.append((T.table(g8), dict(base_time=T.LIMIT - 1 - (len(g8) + 3) * 7, tick=7, delay=3)))
    out.append((T.table(g8), dict(base_time=T.LIMIT - (len(g8) + 3) * 7, tick=7, delay=3)))
    out += [(T.table(g8), kw) for kw in (dict(tick=0), dict(flags=4), dict(reserved=(0, 0, 1)), dict(reserved=(1, 0, 0)), dict(base_time=T.LIMIT),
                                         dict(tick=(1 << 32) - 1, base_time=T.LIMIT - 1, delay=(1 << 32) - 1))]
    # random: near-sorted keys, random heads and AUs without a picture
    for seed in range(6):
        n = int(rng.integers(1, 5 * B))
        keys = T.near_sorted(rng, n, reach=int(rng.integers(1, 60)))
        heads = sorted(set(rng.integers(0, n, int(rng.integers(0, 9))).tolist()))
        nopic = sorted(set(rng.integers(0, n, int(rng.integers(0, 30))).tolist()))
        out.append((T.table(keys, heads=heads, nopic=nopic, junk=rng), dict(tick=int(rng.integers(1, 5000)), base_time=int(rng.integers(0, 1 << 40)))))
    return out


def record(kw):
    kw = dict(kw)
    return T.params_record(**kw)


def test_plan_single_stepped_under_sanitizers(tmp_path):
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
    src = tmp_path / "autimes_host_asan.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "autimes_host_asan"
    cmd = [cxx] + flags + ["-I", os.path.join(ROOT, "hevcbitstream_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    todo = cases()
    with open(tmp_path / "cases.bin", "wb") as f:
        for au, kw in todo:
            f.write(record(kw).tobytes() + struct.pack("<Q", len(au)) + au.tobytes())
    run = subprocess.run([str(exe), str(tmp_path / "cases.bin")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-6000:]
    lines = run.stdout.splitlines()
    assert len(lines) == len(todo)
    verdicts = set()
    for i, ((au, kw), got) in enumerate(zip(todo, lines)):
        assert got == want(au, kw), (i, len(au), kw)
        verdicts.add(got.split()[0])
    assert verdicts == {"ok", "depth", "refused"}
