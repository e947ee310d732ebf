"""The output of a copy call as a list of segments, so that a reference can say what every output byte is without holding the
stream: the plan forms of tests/_rtp_ref.py, tests/_tsmux_ref.py and tests/_auins_ref.py return such lists, materialise() turns
one into bytes over a host stream, and tests/_big.py checks one against tensors of several GiB.  A segment is
  ("copy", out, src, length)   source bytes [src, src + length) at output offset out
  ("lit", out, bytes)          those bytes at out
  ("run", out, run)            run["n"] packets of run["P"] bytes each from out on: run["H"] header bytes, the rows of
                               run["heads"](lo, hi) for packets lo .. hi - 1 of the run; then run["F"] source bytes, packet i's from
                               run["src"] + i * F; then the constant bytes run["tail"]
Segments are in output order and tile [0, total).  numpy only."""
import numpy as np


def seg_bytes(seg):
    if seg[0] == "copy":
        return seg[3]
    if seg[0] == "lit":
        return len(seg[2])
    return seg[2]["n"] * seg[2]["P"]


def tiles(segs, total):
    """do the segments lie back to back from 0 to total?"""
    at = 0
    for seg in segs:
        if seg[1] != at or seg_bytes(seg) <= 0:
            return False
        at += seg_bytes(seg)
    return at == total


def run_of(n, P, H, F, src, heads, tail=b""):
    assert n > 0 and P == H + F + len(tail)
    return dict(n=n, P=P, H=H, F=F, src=src, heads=heads, tail=bytes(tail))


def materialise(segs, total, stream):
    """the bytes of the segments over a host stream"""
    stream = np.frombuffer(stream, dtype=np.uint8) if isinstance(stream, (bytes, bytearray)) else np.asarray(stream, dtype=np.uint8)
    assert tiles(segs, total), "the segments do not tile the output"
    out = np.zeros(total, dtype=np.uint8)
    for seg in segs:
        o = seg[1]
        if seg[0] == "copy":
            out[o:o + seg[3]] = stream[seg[2]:seg[2] + seg[3]]
        elif seg[0] == "lit":
            out[o:o + len(seg[2])] = np.frombuffer(seg[2], dtype=np.uint8)
        else:
            r = seg[2]
            rows = out[o:o + r["n"] * r["P"]].reshape(r["n"], r["P"])
            rows[:, :r["H"]] = r["heads"](0, r["n"])
            rows[:, r["H"]:r["H"] + r["F"]] = stream[r["src"]:r["src"] + r["n"] * r["F"]].reshape(r["n"], r["F"])
            if r["tail"]:
                rows[:, r["H"] + r["F"]:] = np.frombuffer(r["tail"], dtype=np.uint8)
    return out
