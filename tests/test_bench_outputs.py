"""bench.py's --dump-outputs (what the timed path computed in its last step, as .npy files) and the split between a plain
run and --full.  The CPU tests drive bench.dump_outputs with host tensors made by the oracle's generator; the GPU test runs
a small plain bench.py and checks the files it wrote against the same generator (the device's hbs_synth_* makes the same
bytes)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ("summary", "index_rows", "index_sample", "index_block_sums", "rbsp_offsets", "rbsp_sample", "rbsp_block_sums")
FIELDS = ("start", "end", "rbsp_off", "rbsp_len", "status")


def _load(d):
    return {f: np.load(os.path.join(d, f + ".npy")) for f in FILES}


def _block_sums(idx, arena, block):
    n = len(idx)
    cols = np.zeros(((n + 1023) // 1024 * 1024, 5), dtype=np.int64)
    for j, f in enumerate(FIELDS):
        cols[:n, j] = idx[f].astype(np.int64)
    isum = cols.reshape(-1, 1024, 5).sum(axis=1)
    nb = (len(arena) + block - 1) // block
    a = np.zeros(nb * block, dtype=np.int64)
    a[: len(arena)] = arena
    a = a.reshape(nb, block)
    rsum = np.stack([a.sum(axis=1), (a * np.arange(1, block + 1, dtype=np.int64)).sum(axis=1)], axis=1)
    return isum, rsum


def _check_against(d, idx, arena, nal_count, block=1 << 20, fields=FIELDS):
    """the files in d against the generator's index and arena (`fields`: the index fields to compare)"""
    got = _load(d)
    for f in FILES:
        assert got[f].dtype in (np.float32, np.float64), (f, got[f].dtype)
    assert got["summary"][0] == nal_count and got["summary"][2] == len(arena)
    rows = got["index_rows"].astype(np.int64)
    assert np.array_equal(rows, np.unique(rows)) and rows[0] >= 0 and rows[-1] < len(idx)
    cols = [FIELDS.index(f) for f in fields]
    want = np.stack([idx[f][rows].astype(np.float64) for f in fields], axis=1)
    assert np.array_equal(got["index_sample"][:, cols], want)
    offs = got["rbsp_offsets"].astype(np.int64)
    assert np.array_equal(offs, np.sort(offs)) and offs[0] >= 0 and offs[-1] < len(arena)
    assert np.array_equal(got["rbsp_sample"], arena[offs].astype(np.float32))
    isum, rsum = _block_sums(idx, arena, block)
    assert np.array_equal(got["index_block_sums"][:, cols], isum[:, cols].astype(np.float64))
    assert np.array_equal(got["rbsp_block_sums"], rsum.astype(np.float64))
    return got


@pytest.mark.parametrize("n,max_rows,max_bytes,block", [(300, 64, 5000, 4096), (300, 512, 1 << 23, 1 << 20)],
                         ids=["sampled", "whole"])
def test_dump_outputs_on_host_tensors(orc, tmp_path, n, max_rows, max_bytes, block):
    """every file holds what the index / arena / summary it was given hold, at the rows and offsets it names; the sample
    positions are seeded: the same inputs give the same files"""
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from hevcbitstream_amd.api import SUMMARY
    _, idx, arena = orc.gen_stream(0x1234, n, 1)
    s = np.zeros(1, dtype=SUMMARY)[0]
    s["nal_count"], s["nal_found"], s["rbsp_bytes"], s["stream_bytes"], s["stop_reason"], s["error"] = n, n, len(arena), 12345, -1, 0
    index = torch.from_numpy(idx.view(np.uint8).copy())
    rbsp = torch.from_numpy(arena.copy())
    runs = []
    for k in range(2):
        d = str(tmp_path / ("d%d" % k))
        bench.dump_outputs(torch, d, index, rbsp, s, n, len(arena), max_rows=max_rows, max_bytes=max_bytes, block=block)
        runs.append(_check_against(d, idx, arena, n, block=block))
    assert list(runs[0]["summary"]) == [n, n, len(arena), 12345, -1, 0]
    assert len(runs[0]["index_rows"]) == min(n, max_rows) and len(runs[0]["rbsp_offsets"]) == min(len(arena), max_bytes)
    for f in FILES:
        assert np.array_equal(runs[0][f], runs[1][f]), f


def test_bench_options():
    """--full and --dump-outputs are on the command line (argparse runs before anything touches torch or the GPU)"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert "--full" in p.stdout and "--dump-outputs" in p.stdout and "--steps" in p.stdout


@pytest.mark.gpu
def test_plain_bench_run_dumps_the_last_step(orc, tmp_path):
    """a plain run prints the headline line and nothing of --full, takes exactly --steps timed steps, and its dump equals
    what the generator says the index and the arena are"""
    n = 20000
    d = str(tmp_path / "out")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--nals", str(n),
           "--dump-outputs", d]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "GB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert "cpu_baseline" not in line and "other_kernels" not in line
    assert "kernel_ms_plain_arena" not in line["roofline"]
    assert len(line["roofline"]["kernel_ms_steps"]) == 3
    _, idx, arena = orc.gen_stream(0x1234, n, 0)
    # (the status the scan reports for the last NAL is the scan's own business: tests/test_gpu_scan.py)
    got = _check_against(d, idx, arena, n, fields=("start", "end", "rbsp_off", "rbsp_len"))
    assert got["summary"][4] == -1 and got["summary"][5] == 0
    assert sum(os.path.getsize(os.path.join(d, f + ".npy")) for f in FILES) <= 64 << 20
