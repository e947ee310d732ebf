"""hbs_au_times restated from the header comment (include/hevcbitstream_amd.h), not from the kernels: one `sorted` per segment
for the output slot (the first form of o(a)), back(a) / fwd(a) by comparing every pair of a segment, the times in Python
integers.  Also the small generators the tests share: AU tables from lists of picture order counts, B-pyramids, near-sorted
random tables."""
import numpy as np

from hevcbitstream_amd.api import ACCESS_UNIT, AU_TIMES_PARAMS

MAX_SPAN = 1024
DELAY_GIVEN, WRAP33 = 1, 2
CVS_START, NO_PICTURE = 4, 16
E_ARG, E_DEPTH = -3, -6
LIMIT = 1 << 62
NONE = -(1 << 31)


def table(pocs, heads=(), nopic=(), junk=None):
    """ndarray[ACCESS_UNIT]: pic_order_cnt from `pocs`, HBS_AU_CVS_START on the AUs in `heads`, HBS_AU_NO_PICTURE on those in
    `nopic`; with `junk` (a Generator) every field the call does not read, and every flag bit it does not look at, is random"""
    n = len(pocs)
    au = np.zeros(n, dtype=ACCESS_UNIT)
    if junk is not None and n:
        au.view(np.uint8)[:] = junk.integers(0, 256, n * ACCESS_UNIT.itemsize, dtype=np.uint8)
        au["flags"] &= ~np.uint32(CVS_START | NO_PICTURE)
    au["pic_order_cnt"] = np.asarray(pocs, dtype=np.int64).astype(np.int32)
    for a in heads:
        au["flags"][a] |= CVS_START
    for a in nopic:
        au["flags"][a] |= NO_PICTURE
    return au


def params_record(tick=1, base_time=0, delay=None, flags=0, reserved=(0, 0, 0)):
    p = np.zeros(1, dtype=AU_TIMES_PARAMS)
    p["flags"], p["tick"], p["base_time"] = flags | (DELAY_GIVEN if delay is not None else 0), tick, base_time
    p["delay"] = 0 if delay is None else delay
    p["reserved"][0] = reserved
    return p


def refused(n_aus, tick=1, base_time=0, delay=None, flags=0, reserved=(0, 0, 0)):
    """what the call refuses at once, of the things a params record can say"""
    given = delay is not None or bool(flags & DELAY_GIVEN)
    if (flags & ~(DELAY_GIVEN | WRAP33)) or any(reserved) or tick == 0 or base_time >= LIMIT or n_aus > (1 << 32) - 1:
        return True
    d = (delay or 0) if given else MAX_SPAN
    return base_time + (n_aus + d) * tick >= LIMIT


def heads_of(au):
    n = len(au)
    return [a for a in range(n) if a == 0 or int(au["flags"][a]) & CVS_START]


def segments(au):
    """[(first AU, one past the last)]"""
    h = heads_of(au)
    return list(zip(h, h[1:] + [len(au)]))


def keys(au):
    out, last = [], NONE
    for f, poc in zip(au["flags"].tolist(), au["pic_order_cnt"].tolist()):
        if not f & NO_PICTURE:
            last = poc
        out.append(last)
    return out


def order(au):
    key = keys(au)
    o = [0] * len(au)
    for s, e in segments(au):
        for rank, b in enumerate(sorted(range(s, e), key=lambda b: (key[b], b))):
            o[b] = s + rank
    return o


def spans(au):
    """(back, fwd) per AU, by brute force: every pair of a segment"""
    key = np.asarray(keys(au), dtype=np.int64)
    back, fwd = np.zeros(len(au), dtype=np.int64), np.zeros(len(au), dtype=np.int64)
    for s, e in segments(au):
        k, L = key[s:e], e - s
        at = np.arange(L)
        for lo in range(0, L, 2048):                       # rows lo .. hi of the L x L comparison at a time
            hi = min(lo + 2048, L)
            rows = at[lo:hi, None]
            higher_in_front = (k[None, :] > k[lo:hi, None]) & (at[None, :] < rows)
            lower_behind = (k[None, :] < k[lo:hi, None]) & (at[None, :] > rows)
            back[s + lo:s + hi] = np.where(higher_in_front.any(1), at[lo:hi] - higher_in_front.argmax(1), 0)
            fwd[s + lo:s + hi] = np.where(lower_behind.any(1), L - 1 - lower_behind[:, ::-1].argmax(1) - at[lo:hi], 0)
    return back, fwd


def au_times(au, tick=1, base_time=0, delay=None, flags=0):
    """-> dict(dts, pts, order, display: ndarrays, or None on the error; summary: dict)"""
    assert not refused(len(au), tick, base_time, delay, flags)
    n = len(au)
    back, fwd = spans(au)
    bad = np.flatnonzero((back > MAX_SPAN) | (fwd > MAX_SPAN))
    if len(bad):
        return dict(dts=None, pts=None, order=None, display=None,
                    summary=dict(nal_count=0, nal_found=0, rbsp_bytes=0, stream_bytes=0, stop_reason=0, error=E_DEPTH,
                                 reserved=[1 + int(bad[0]), 0, 0]))
    o = order(au)
    assert sorted(o) == list(range(n))
    R = max([a - o[a] for a in range(n)] + [0])
    d = delay if delay is not None else R
    wrap = (lambda t: t % (1 << 33)) if flags & WRAP33 else (lambda t: t)
    dts = [base_time + a * tick for a in range(n)]
    pts = [base_time + (o[a] + d) * tick for a in range(n)]
    display = [0] * n
    for a in range(n):
        display[o[a]] = a
    h = heads_of(au)
    late = sum(1 for a in range(n) if pts[a] < dts[a])
    return dict(dts=np.array([wrap(t) for t in dts], dtype=np.uint64), pts=np.array([wrap(t) for t in pts], dtype=np.uint64),
                order=np.array(o, dtype=np.uint32), display=np.array(display, dtype=np.uint32), exact_dts=dts, exact_pts=pts,
                summary=dict(nal_count=n, nal_found=len(h), rbsp_bytes=h[-1] if h else 0, stream_bytes=0, stop_reason=0, error=0,
                             reserved=[d, R, late]))


# ---- generators ----

def pyramid(gop, gops, first=0):
    """decode-order POCs of an IDR and `gops` B-pyramids of `gop` pictures: the anchor, then the middles, depth first"""
    def mid(lo, hi):
        m = (lo + hi) // 2
        return [] if m == lo else [m] + mid(lo, m) + mid(m, hi)
    out = [first]
    for g in range(gops):
        out += [first + (g + 1) * gop] + mid(first + g * gop, first + (g + 1) * gop)
    return out


def near_sorted(rng, n, reach=32):
    """n keys with ties, each displaced by fewer than `reach` positions from sorted order, so that no span passes 2 * reach"""
    base = np.arange(n, dtype=np.int64) + rng.integers(0, reach, n)
    return (base // 2 - n // 4).tolist()                  # ties (// 2) and negative keys
