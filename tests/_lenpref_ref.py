"""Plain-loop reference of hbs_annexb_to_lenpref / hbs_lenpref_to_annexb (include/hevcbitstream_amd.h): the specification
restated, byte by byte.  Test infrastructure only."""
import numpy as np

from tests._filter_ref import NAL_ENTRY, ST_UNTERMINATED, E_ARG, E_CAPACITY, consistent   # noqa: F401

SC = {3: b"\x00\x00\x01", 4: b"\x00\x00\x00\x01"}


def au_table_ok(nal_au, n_nals, n_aus):
    """d_nal_au[0] == 0, steps of 0 or +1, d_nal_au[-1] == n_aus - 1; no NALs: no AUs"""
    if n_nals == 0:
        return n_aus == 0
    a = [int(x) for x in nal_au]
    if a[0] != 0 or a[-1] != n_aus - 1:
        return False
    return all(a[k] - a[k - 1] in (0, 1) for k in range(1, n_nals))


def to_lenpref_ref(stream, idx, keep=None, L=4, nal_au=None, n_aus=0, out_cap=None):
    """-> (out bytes, index_out, sample_off or None, summary dict).  On an error: no bytes, no entries, no table."""
    s = np.asarray(stream, dtype=np.uint8)
    n = len(idx)
    keep = np.ones(n, dtype=bool) if keep is None else np.asarray(keep).astype(bool)
    summ = dict(nal_count=0, nal_found=n, rbsp_bytes=0, stream_bytes=0, stop_reason=0, error=0)
    none = (np.zeros(0, np.uint8), np.zeros(0, dtype=NAL_ENTRY), None)
    bad = False
    prev_end = 0
    kept = []
    starts, ends, rlens, stats = (idx[f].tolist() for f in ("start", "end", "rbsp_len", "status"))
    for k in range(n):
        st, en = starts[k], ends[k]
        ok = st <= en and en <= len(s) and st >= prev_end        # each entry is checked before it is used
        prev_end = en
        if not ok:
            bad = True
            continue
        if keep[k]:
            if en - st > (1 << (8 * L)) - 1:
                bad = True
                continue
            kept.append(k)
    if nal_au is not None and not au_table_ok(nal_au, n, n_aus):
        bad = True
    if bad:
        summ["error"] = E_ARG
        return none + (summ,)
    sb = s.tobytes()
    out = bytearray()
    o_start, o_end, o_roff = [], [], []
    au_bytes = [0] * n_aus                  # record bytes of the kept NALs of each AU
    roff = 0
    for k in kept:
        st, en = starts[k], ends[k]
        out += (en - st).to_bytes(L, "big")
        o_start.append(len(out))
        out += sb[st:en]
        o_end.append(len(out))
        o_roff.append(roff)
        roff += rlens[k]
        if nal_au is not None:
            au_bytes[int(nal_au[k])] += L + en - st
    io = np.zeros(len(kept), dtype=NAL_ENTRY)
    io["start"], io["end"], io["rbsp_off"] = o_start, o_end, o_roff
    io["rbsp_len"] = [rlens[k] for k in kept]
    io["status"] = [stats[k] & ~ST_UNTERMINATED for k in kept]
    summ.update(nal_count=len(kept), rbsp_bytes=roff, stream_bytes=len(out))
    if out_cap is not None and out_cap < len(out):
        summ["error"] = E_CAPACITY
        return none + (summ,)
    sample_off = None
    if nal_au is not None:                  # the AU numbers never step back: "kept NALs k with nal_au[k] < a" are the AUs in front of a
        sample_off = np.zeros(n_aus + 1, dtype=np.uint64)
        for a in range(n_aus):
            sample_off[a + 1] = int(sample_off[a]) + au_bytes[a]
    return np.frombuffer(bytes(out), dtype=np.uint8).copy(), io, sample_off, summ


def to_annexb_ref(data, off, size, L=4, sc=4, nal_cap=None, out_cap=None):
    """-> (out bytes, sample_off_out, summary dict; summary["reserved0"] = 1 + the lowest bad sample, or 0).  On an error: no
    bytes and no table."""
    d = np.asarray(data, dtype=np.uint8).tobytes()
    n = len(off)
    out = bytearray()
    starts = []
    recs = 0
    total = 0
    bad = 0
    for s_ in range(n):
        o, z = int(off[s_]), int(size[s_])
        starts.append(total)
        if o + z >= (1 << 64) or o + z > len(d):
            bad = bad or s_ + 1
            continue
        p, e = o, o + z
        while p < e:
            if e - p < L:
                bad = bad or s_ + 1
                break
            ln = int.from_bytes(d[p:p + L], "big")
            p += L
            if ln > e - p:
                bad = bad or s_ + 1
                break
            out += SC[sc] + d[p:p + ln]
            p += ln
            recs += 1
            total += sc + ln
    starts.append(total)
    summ = dict(nal_count=recs, nal_found=n, rbsp_bytes=0, stream_bytes=total, stop_reason=-1 if recs else 0, error=0, reserved0=bad)
    err = E_ARG if bad else E_CAPACITY if (nal_cap is not None and recs > nal_cap) or (out_cap is not None and out_cap < total) else 0
    if err:
        summ["error"] = err
        return np.zeros(0, np.uint8), None, summ
    return np.frombuffer(bytes(out), dtype=np.uint8).copy(), np.array(starts, dtype=np.uint64), summ


def rescan_misses_last(out, payloads, sc):
    """The stated exception of a find_nal_unit walk over hbs_lenpref_to_annexb's output (payloads: what was written, in order):
    a last record of length 0 behind a 3-byte start code, with a record in front of it.  The walk's `i+3 >= size` rule ends
    the payload in front at the buffer's end before the last start code is looked at: the last record is not found and the
    one in front comes out three bytes longer."""
    return len(payloads) >= 2 and len(payloads[-1]) == 0 and sc == 3
