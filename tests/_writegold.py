"""What the reference's writer recorded in tests/golden/write_vectors.json.gz, laid out for a whole batch: one row per NAL
with the RBSP bytes, the result record and the struct edits the golden script made; and the two helpers every user of
those vectors needs (field_index, slot_bytes).  Used by tests/test_sim_write.py (CPU), tests/test_gpu_write.py and the
generator tests/golden/make_golden_write.py.  Every expected byte comes from the reference's `out` (its NAL, back to RBSP with
nal_to_rbsp); nothing here is taken from the code under test."""
import gzip
import json
import os

import numpy as np

from tests import _orc
from tests._parsecmp import which_struct

HERE = os.path.dirname(os.path.abspath(__file__))
_vectors = None
_caps = None
_fields = {}

TILES = 40          # tests/test_gpu_write.py writes the ten sequences as one batch, up to this many times over
# (seed, step) of the steps that do NOT parse, inside that batch, to the rc and struct they have when their sequence is parsed
# alone -- each with its reason.  tests/test_sim_write.py finds them on the CPU; neither test compares them.  None does.
LEFT_OUT = ()


def vectors():
    global _vectors
    if _vectors is None:
        _vectors = json.load(gzip.open(os.path.join(HERE, "golden", "write_vectors.json.gz"), "rt"))
    return _vectors


def caps_fixture():
    """tests/golden/write_caps.json.gz: {seed: {k: step}} (make_golden_write.py --caps)"""
    global _caps
    if _caps is None:
        raw = json.load(gzip.open(os.path.join(HERE, "golden", "write_caps.json.gz"), "rt"))
        _caps = {v["seed"]: {s["k"]: s for s in v["steps"]} for v in raw}
    return _caps


def rows_fixture():
    """tests/golden/write_rows.json.gz: a slice whose bytes depend on the RPS row it is handed (make_golden_write.py --rows)"""
    return json.load(gzip.open(os.path.join(HERE, "golden", "write_rows.json.gz"), "rt"))


def field_index(kind, name):
    if kind not in _fields:
        _fields[kind] = {n: i for n, i, c in _orc.flat_fields(_orc.STRUCT_TYPES[kind])}
    return _fields[kind][name]


def slot_bytes(kind):
    size = _orc.layout()[_orc.STRUCT_TYPES[kind]]["size"]
    if kind == "sps":      # + hbs::RpsTables: three counts and four rows of 32 ints for each of 32 sets (test_gpu_write holds it to hbs_sps_slot_bytes())
        return ((size + 15) // 16) * 16 + 4 * (3 * 32 + 4 * 32 * 32)
    return ((size + 15) // 16) * 16


class Gold:
    """The steps of one or several golden sequences, one after the other, as one batch of n NALs.
    nals[k]; kind[k] ('vps' / 'sps' / 'pps' / 'sh' / None); read_rc[k]; has[k]: the reference wrote it;
    rbsp[k] (bytes) and L[k] = len(rbsp[k]); ref_cap[k] = size * 3 // 4, the reference's own RBSP buffer (hevc_stream.c:1266);
    sds[k]: what it left in h->slice_data->rbsp_size with that buffer; edits[k] = [(int32 index in the struct, value)];
    edited_set[k]: a parameter set that the golden script edited."""

    def __init__(self, seqs):
        orc = _orc.oracle()
        steps = [st for v in seqs for st in v["steps"]]
        self.left_out = np.array([(v["seed"], k) in LEFT_OUT for v in seqs for k in range(len(v["steps"]))])
        self.steps = steps
        self.n = n = len(steps)
        self.nals = [bytes.fromhex(st["nal"]) for st in steps]
        self.type = np.array([(nal[0] >> 1) & 0x3F for nal in self.nals])
        self.kind = [which_struct(int(t)) for t in self.type]
        self.read_rc = np.array([st["read_rc"] for st in steps])
        self.has = np.array(["write_rc" in st for st in steps])
        self.rbsp, self.edits = [], []
        self.L = np.zeros(n, dtype=np.int64)
        self.ref_cap = np.zeros(n, dtype=np.int64)
        self.sds = np.zeros(n, dtype=np.int64)
        for k, st in enumerate(steps):
            rb, ed = b"", []
            if self.has[k]:
                assert st["write_rc"] >= 0
                rc, _, _, rb = orc.nal_to_rbsp(bytes.fromhex(st["out"]))
                assert rc == len(rb)
                ed = [(field_index(self.kind[k], name), value) for name, value in st["edits"]]
                self.ref_cap[k] = st["size"] * 3 // 4
                self.sds[k] = st["slice_data_size"]
            self.rbsp.append(rb)
            self.edits.append(ed)
            self.L[k] = len(rb)
        self.is_slice = np.array([kd == "sh" for kd in self.kind])
        self.is_set = np.array([kd in ("vps", "sps", "pps") for kd in self.kind])
        self.edited = np.array([len(e) > 0 for e in self.edits])
        self.edited_set = self.is_set & self.edited
        self._tables = {}
        self.on_device = {}              # a user's cache of table(cap) on a device
        self.unwritten = np.array([kd is None for kd in self.kind])          # AUD, SEI: write_hevc_nal_unit returns -1 (:1315)

    def default_cap(self):
        return int(max(st["size"] for st in self.steps if "size" in st)) * 3 // 4

    def slot_extent(self, parsed, n, of=None):
        """bytes of the struct arena that the first n NALs of `parsed` use"""
        of = np.arange(self.n) if of is None else np.asarray(of)
        size = np.array([slot_bytes(kd) if kd else 0 for kd in self.kind], dtype=np.int64)[of[:n]]
        off = parsed["struct_off"][:n]
        ok = (off != np.uint64(0xFFFFFFFFFFFFFFFF)) & (size > 0)
        return int((off[ok].astype(np.int64) + size[ok]).max())

    def table(self, cap):
        """[n, cap] uint8: row k = the first `cap` bytes of the reference's RBSP, zeros behind (the writer's buffer is
        calloc'ed, :1255, and bs.h's put drops what does not fit but keeps counting)"""
        if cap not in self._tables:
            t = np.zeros((self.n, cap), dtype=np.uint8)
            for k, rb in enumerate(self.rbsp):
                m = min(len(rb), cap)
                t[k, :m] = np.frombuffer(rb[:m], dtype=np.uint8)
            self._tables[cap] = t
        return self._tables[cap]

    def sds_at(self, cap):
        """h->slice_data->rbsp_size is b->end - (b->p + 1) (:1702-1703) with b->end = buffer + size * 3 / 4: what the
        reference recorded with ITS buffer, moved by the difference to a buffer of `cap` bytes.  Slices only."""
        return np.where(self.is_slice & self.has, self.sds + (cap - self.ref_cap), 0)

    def edit_lists(self, parsed, which, of=None):
        """(int32 indices into the struct arena, values) of the edits of the steps in mask `which` (over the steps);
        of[j]: the step that NAL j of `parsed` is (default: NAL j is step j).  No loop over the NALs."""
        of = np.arange(self.n) if of is None else np.asarray(of)
        width = max([len(e) for e in self.edits] + [1])
        fi = np.full((self.n, width), -1, dtype=np.int64)
        fv = np.zeros((self.n, width), dtype=np.int32)
        for k, e in enumerate(self.edits):
            for j, (i, v) in enumerate(e):
                fi[k, j], fv[k, j] = i, v
        take = (fi[of] >= 0) & np.asarray(which)[of][:, None]
        off = parsed["struct_off"][:len(of)].astype(np.int64)
        assert (off[take.any(1)] >= 0).all() and (off[take.any(1)] % 4 == 0).all()
        idx = off[:, None] // 4 + fi[of]
        return idx[take], fv[of][take]

    def sets_in_force(self):
        """(sps[k], pps[k]): the last SPS / PPS NAL in front of NAL k in this batch, -1: none"""
        sps = np.full(self.n, -1, dtype=np.int64)
        pps = np.full(self.n, -1, dtype=np.int64)
        s = p = -1
        for k in range(self.n):
            sps[k], pps[k] = s, p
            if self.type[k] == 33:
                s = k
            elif self.type[k] == 34:
                p = k
        return sps, pps
