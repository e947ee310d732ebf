#!/usr/bin/env python3
"""Golden vectors for the syntax writers: the reference's write_hevc_nal_unit (hevc_stream.c:1249-1327)
run in this container on parsed (and on edited) structs.  Needs oracle/_ref/libhevcref.so.

For every NAL of a few synthetic sequences: read it with the reference, optionally edit a field of the
parsed struct, write it back with the reference into a buffer of `size` bytes; recorded: the bytes
written, the return value and what the writer left in h->slice_data->rbsp_size.

usage: python tests/golden/make_golden_write.py   ->  tests/golden/write_vectors.json.gz
       python tests/golden/make_golden_write.py --caps   ->  tests/golden/write_caps.json.gz
       python tests/golden/make_golden_write.py --rows   ->  tests/golden/write_rows.json.gz

--rows: one slice whose bytes depend on the RPS row it is handed.  No step of write_vectors.json.gz does (an IDR there is an
I slice or a dependent segment).  In a fresh process, so that the reference's file-static tables (:26-32) are still zero
behind the SPS's own sets: seed 10's VPS, SPS and second PPS (lists_modification_present_flag = 1) are read, then its IDR
step 8, whose slice_type is set to P, is written.  A P-type IDR codes no st_ref_pic_set and counts the used pictures of row
num_short_term_ref_pic_sets (:35-59), which nothing has written: the recorded bytes are those of an all-zero row.  Step 10
goes into the fixture as a NAL only: the test turns it into a slice that leaves a row with used pictures.

--caps: what the reference answers when the buffer is just about too small.  For the sequences of
write_vectors.json.gz (which has to exist; it is read, not written) and every step written WITHOUT an edit, with L
the RBSP length of the recorded output: write_hevc_nal_unit with the `size` values whose size * 3 / 4 (:1265) is
L - 1, L, L + 1 and L + 2, into a buffer with guard bytes behind `size`.  Recorded per step: k, L, the four sizes,
their size * 3 / 4 and the four return values; null where the reference did not return.  The four writes come in
front of the write of the golden flow, which is then checked against write_vectors.json.gz: the extra writes do
not change what the reference holds.

What the reference does at these sizes (found with this script):
  - size * 3 / 4 == L - 1 on a slice: it does not return.  write_hevc_slice_layer_rbsp (:1702-1706) copies
    b->end - (b->p + 1) bytes of "slice data", here -1: malloc fails and memcpy faults.  Those entries are null;
    one process per sequence, started again behind each such entry with the entries already known handed in.
  - everywhere else it returns, the guard bytes are intact, and the return value is negative exactly where
    size * 3 / 4 < L (bs_overrun, :1319); at L and above the NAL always fitted `size` (rbsp_to_nal, :1326).
"""
import ctypes as C
import gzip
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import _orc                                           # noqa: E402
from tests._parsecmp import which_struct                         # noqa: E402
from tests._writegold import field_index                         # noqa: E402
from tests.test_sim_parse_logic import sequence                  # noqa: E402

EDITS = {  # struct kind -> [(field, delta)] applied to every second NAL of that kind
    "sps": [("pic_width_in_luma_samples", 16), ("log2_max_pic_order_cnt_lsb_minus4", 1)],
    "pps": [("init_qp_minus26", -3), ("pps_cb_qp_offset", 2)],
    "sh": [("slice_qp_delta", 5), ("slice_type", 0)],
    "vps": [("vps_max_layer_id", 1)],
}


def one(seed):
    if True:
        nals = sequence(seed)
        r = _orc.ReferenceHevc()
        steps = []
        seen = {}
        for nal in nals:
            rc = r.read(nal)
            t = int(r.v["nal"][1])
            kind = which_struct(t)
            step = {"nal": bytes(nal).hex(), "read_rc": rc}
            if rc >= 0 and kind is not None:
                seen[kind] = seen.get(kind, 0) + 1
                edits = []
                saved = r.v[kind].copy()
                if seen[kind] % 2 == 0:
                    for name, delta in EDITS[kind]:
                        i = field_index(kind, name)
                        new = int(r.v[kind][i]) + delta if name != "slice_type" else 2       # I slice: no ref lists
                        r.v[kind][i] = new
                        edits.append([name, new])
                size = 2 * len(nal) + 64
                out = np.zeros(size + 16, dtype=np.uint8)
                wrc = r.L.write_hevc_nal_unit(r.h, out.ctypes.data_as(C.POINTER(C.c_uint8)), size)
                r.v[kind][:] = saved          # the edit is for this write only: later NALs are read against the stream's own structs
                step.update({"edits": edits, "size": size, "write_rc": int(wrc),
                             "out": bytes(out[:max(wrc, 0)]).hex(), "slice_data_size": int(r.slice_data()[0])})
            steps.append(step)
        return {"seed": seed, "steps": steps}


GUARD = 64


def size_for(cap):
    """the smallest `size` with size * 3 // 4 == cap"""
    s = (4 * cap + 2) // 3
    assert s * 3 // 4 == cap and (s - 1) * 3 // 4 < cap
    return s


def caps_one(seed, gold_steps, known):
    """One sequence, in this process: a JSON line per write, flushed, so that the parent knows how far it came.
    known: {(k, size): rc or None} from earlier starts; those writes are not made again."""
    orc = _orc.oracle()
    nals = sequence(seed)
    assert [bytes(n).hex() for n in nals] == [s["nal"] for s in gold_steps]
    r = _orc.ReferenceHevc()
    u8p = C.POINTER(C.c_uint8)
    for k, (nal, st) in enumerate(zip(nals, gold_steps)):
        rc = r.read(nal)
        assert rc == st["read_rc"]
        if "write_rc" not in st:
            continue
        kind = which_struct(int(r.v["nal"][1]))
        saved = r.v[kind].copy()
        if not st["edits"]:
            L = len(orc.nal_to_rbsp(bytes.fromhex(st["out"]))[3])
            for cap in (L - 1, L, L + 1, L + 2):
                size = size_for(cap)
                if (k, size) in known:
                    continue
                print(json.dumps({"k": k, "L": L, "size": size, "cap": cap, "begin": 1}), flush=True)
                out = np.full(size + GUARD, 0xC3, dtype=np.uint8)
                wrc = int(r.L.write_hevc_nal_unit(r.h, out.ctypes.data_as(u8p), size))
                inside = bool((out[size:] == 0xC3).all()) and wrc <= size
                print(json.dumps({"k": k, "L": L, "size": size, "cap": cap, "rc": wrc, "inside": inside}), flush=True)
        for name, value in st["edits"]:
            r.v[kind][field_index(kind, name)] = value
        out = np.zeros(st["size"] + 16, dtype=np.uint8)
        wrc = int(r.L.write_hevc_nal_unit(r.h, out.ctypes.data_as(u8p), st["size"]))
        r.v[kind][:] = saved
        assert wrc == st["write_rc"] and bytes(out[:max(wrc, 0)]).hex() == st["out"], ("golden flow", k)
        assert int(r.slice_data()[0]) == st["slice_data_size"], ("golden flow", k)
    print(json.dumps({"done": 1}), flush=True)


def caps_main():
    import subprocess
    gold = json.load(gzip.open(os.path.join(HERE, "write_vectors.json.gz"), "rt"))
    result = []
    for v in gold:
        known = {}
        meta = {}
        for start in range(400):
            arg = json.dumps([[k, s, rc] for (k, s), rc in known.items()])
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--caps-seed", str(v["seed"]), arg],
                               stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
            lines = [json.loads(x) for x in p.stdout.decode().splitlines() if x.startswith("{")]
            done = False
            pending = None
            for ln in lines:
                if "done" in ln:
                    done = True
                elif "begin" in ln:
                    pending = ln
                else:
                    assert ln["inside"], ("the reference wrote past `size`", v["seed"], ln)
                    known[(ln["k"], ln["size"])] = ln["rc"]
                    meta[(ln["k"], ln["size"])] = (ln["L"], ln["cap"])
                    pending = None
            if done:
                break
            assert pending is not None, ("the sequence stopped outside a write", v["seed"], p.returncode)
            known[(pending["k"], pending["size"])] = None          # the reference did not return from this one
            meta[(pending["k"], pending["size"])] = (pending["L"], pending["cap"])
        else:
            raise SystemExit("seed %d: no end" % v["seed"])
        steps = {}
        for (k, size), rc in sorted(known.items()):
            L, cap = meta[(k, size)]
            e = steps.setdefault(k, {"k": k, "L": L, "sizes": [], "caps": [], "rc": []})
            e["sizes"].append(size); e["caps"].append(cap); e["rc"].append(rc)
        result.append({"seed": v["seed"], "steps": [steps[k] for k in sorted(steps)]})
    with gzip.GzipFile(os.path.join(HERE, "write_caps.json.gz"), "wb", mtime=0) as f:
        f.write(json.dumps(result).encode())
    flat = [rc for v in result for s in v["steps"] for rc in s["rc"]]
    print("sequences", len(result), "steps", sum(len(v["steps"]) for v in result), "writes", len(flat),
          "did not return", sum(rc is None for rc in flat))


ROWS_SEED, ROWS_STEPS, ROWS_READER = 10, (0, 1, 7, 8, 10), 3           # VPS, SPS, second PPS, the IDR, a slice with an own set


def rows_one():
    nals = sequence(ROWS_SEED)
    r = _orc.ReferenceHevc()
    for j, k in enumerate(ROWS_STEPS[:ROWS_READER + 1]):
        assert r.read(nals[k]) >= 0
    assert int(r.v["nal"][1]) == 19 and int(r.v["pps"][field_index("pps", "lists_modification_present_flag")]) == 1
    assert int(r.v["sh"][field_index("sh", "dependent_slice_segment_flag")]) == 0
    edits = [["slice_type", 1]]
    for name, value in edits:
        r.v["sh"][field_index("sh", name)] = value
    size = 2 * len(nals[ROWS_STEPS[ROWS_READER]]) + 64
    out = np.zeros(size + 16, dtype=np.uint8)
    wrc = int(r.L.write_hevc_nal_unit(r.h, out.ctypes.data_as(C.POINTER(C.c_uint8)), size))
    assert wrc >= 0 and not out[size:].any()
    print(json.dumps({"seed": ROWS_SEED, "nals": [bytes(nals[k]).hex() for k in ROWS_STEPS], "reader": ROWS_READER, "edits": edits,
                      "size": size, "write_rc": wrc, "out": bytes(out[:wrc]).hex(), "slice_data_size": int(r.slice_data()[0])}))


def main():
    import subprocess
    if len(sys.argv) > 1 and sys.argv[1] == "--rows-one":
        rows_one()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "--rows":
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--rows-one"], stdout=subprocess.PIPE, check=True)
        with gzip.GzipFile(os.path.join(HERE, "write_rows.json.gz"), "wb", mtime=0) as f:
            f.write(p.stdout.decode().strip().splitlines()[-1].encode())
        return
    if len(sys.argv) > 1 and sys.argv[1] == "--caps":
        caps_main()
        return
    if len(sys.argv) > 3 and sys.argv[1] == "--caps-seed":
        gold = json.load(gzip.open(os.path.join(HERE, "write_vectors.json.gz"), "rt"))
        seed = int(sys.argv[2])
        caps_one(seed, [v for v in gold if v["seed"] == seed][0]["steps"],
                 {(k, s): rc for k, s, rc in json.loads(sys.argv[3])})
        return
    if len(sys.argv) > 2 and sys.argv[1] == "--seed":
        print(json.dumps(one(int(sys.argv[2]))))
        return
    vectors = []
    for seed in range(1, 40):
        # the reference's writer can crash on streams outside its envelope: one process per sequence
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--seed", str(seed)], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
        if p.returncode == 0:
            vectors.append(json.loads(p.stdout.decode().strip().splitlines()[-1]))
        if len(vectors) == 10:
            break
    with gzip.open(os.path.join(HERE, "write_vectors.json.gz"), "wt") as f:
        json.dump(vectors, f)
    print("sequences", len(vectors), "written NALs", sum(1 for v in vectors for s in v["steps"] if "write_rc" in s))


if __name__ == "__main__":
    main()
