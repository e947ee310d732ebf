"""hbs_cbcs_crypt on the GPU against tests/_cbcs_ref.py.  Every case compares every byte of the buffer with the reference -- the
canary bytes between and around the samples included -- and every summary field, in both directions; no tolerances.  The kernel
walks the entries 256 a step in 1 024 ranges (kCencRanges: hbs_cenc.h); an entry of fewer than 64 crypt blocks is one lane's, a
longer one a wavefront's when decrypting (kCbcsLaneBlocks: hbs_cbcs.h)."""
import ctypes as C

import numpy as np
import pytest

from tests import _carve as K
from tests import _cbcs_ref as R

pytestmark = pytest.mark.gpu
CAN = 0xC3
H = bytes.fromhex
RANGES, LANE_BLOCKS = 1024, 64
KEY_38A = H("2b7e151628aed2a6abf7158809cf4f3c")
PLAIN_38A = H("6bc1bee22e409f96e93d7e117393172a" "ae2d8a571e03ac9c9eb76fac45af8e51" "30c81c46a35ce411e5fbc1191a0a52ef" "f69f2445df4f9b17ad2b417be66c3710")
CBC_38A = H("7649abac8119b246cee98e9b12e9197d" "5086cb9b507219ee95db113a917678b2" "73bed6b8e3c1743b7116e69e22229516" "3ff1caa1681fac09120eca307586e1a7")
PATTERNS = ((1, 9), (1, 0), (0, 0), (3, 7), (2, 1), (15, 15))
NAL_ENTRY = np.dtype([("start", "<u8"), ("end", "<u8"), ("rbsp_off", "<u8"), ("rbsp_len", "<u4"), ("status", "<i4")])


@pytest.fixture(scope="module")
def ctx():
    import hevcbitstream_amd as hbs
    c = hbs.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(a.copy()).cuda() if a.size else torch.zeros(64, dtype=torch.uint8, device="cuda")


def fresh_summary():
    import torch
    from hevcbitstream_amd.api import SUMMARY
    return torch.full((SUMMARY.itemsize,), 0x5A, dtype=torch.uint8, device="cuda")


def summary_dict(s):
    return dict(error=int(s["error"]), nal_count=int(s["nal_count"]), nal_found=int(s["nal_found"]), rbsp_bytes=int(s["rbsp_bytes"]),
                stream_bytes=int(s["stream_bytes"]), stop_reason=int(s["stop_reason"]), reserved=[int(x) for x in s["reserved"]])


def summary_matches(s, want):
    assert summary_dict(s) == want


def layout(entries_per_sample, gaps, lead=0):
    """samples laid one behind the other with `gaps` bytes between them -> (data_bytes, off, size, first, sub)"""
    off, size, first, subs, at = [], [], [0], [], lead
    for e, gap in zip(entries_per_sample, gaps):
        z = sum(a + b for a, b in e)
        off.append(at)
        size.append(z)
        subs += list(e)
        first.append(len(subs))
        at += z + gap
    return (at, np.array(off, dtype=np.uint64), np.array(size, dtype=np.uint64), np.array(first, dtype=np.uint64),
            np.array(subs, dtype=R.SUBSAMPLE).reshape(-1))


class Crypt:
    """one set of device buffers for hbs_cbcs_crypt (the call wants d_data itself aligned: the samples' offsets carry the odd
    addresses), and the reference's answer for them"""

    def __init__(self, data, off, size, first, sub, key, iv=None, iv0=None, c=1, k=9, whole=False, decrypt=False):
        import torch
        self.host = (np.array(data, dtype=np.uint8), off, size, first, sub)
        self.key, self.iv, self.iv0, self.c, self.k, self.whole = key, iv, iv0, c, k, whole
        self.n = len(off)
        self.d_data = dev(self.host[0])
        self.d_off, self.d_size, self.d_first, self.d_sub = dev(off), dev(size), dev(first), dev(sub)
        self.d_iv = dev(iv) if iv is not None else torch.full((max(self.n, 1) * 16,), CAN, dtype=torch.uint8, device="cuda")
        self.summary = fresh_summary()
        self.direction(decrypt)

    def direction(self, decrypt):
        import hevcbitstream_amd as hbs
        self.decrypt = decrypt
        self.prm = hbs.cbcs_params(self.key, iv0=self.iv0, flags=(hbs.CBCS_DECRYPT if decrypt else 0) | (hbs.CBCS_WHOLE_RUNS if self.whole else 0),
                                   crypt_byte_block=self.c, skip_byte_block=self.k)
        self.summary.fill_(0x5A)

    def launch(self, ctx, iv="own"):
        return ctx.cbcs_crypt_async(self.d_data, len(self.host[0]), self.d_off, self.d_size, self.n, self.d_first, self.d_sub,
                                    self.d_iv if iv == "own" else iv, self.prm, self.summary)

    def data(self):
        return self.d_data[: len(self.host[0])].cpu().numpy()

    def want(self, data=None):
        data, off, size, first, sub = (self.host[0] if data is None else data,) + self.host[1:]
        return R.crypt_many(data, off, size, first, sub, self.key, iv=self.iv, iv0=self.iv0 if self.iv is None else None, c=self.c, k=self.k,
                            whole=self.whole, decrypt=self.decrypt)

    def check(self, ctx, before=None, want=None):
        """the buffer and the summary behind one successful call on `before` (default: what was uploaded)"""
        want, done = self.want(before) if want is None else want
        assert summary_dict(ctx.read_summary(self.summary)) == dict(error=0, nal_count=len(self.host[4]), nal_found=self.n, rbsp_bytes=done,
                                                                    stream_bytes=len(self.host[0]), stop_reason=0, reserved=[0, 0, 0])
        got = self.data()
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
        return want

    def there_and_back(self, ctx):
        """encrypt against the reference, then decrypt what the device holds against the reference and the plaintext"""
        self.direction(False)
        assert self.launch(ctx) == 0
        enc = self.check(ctx)
        self.direction(True)
        assert self.launch(ctx) == 0
        self.check(ctx, before=enc)
        assert np.array_equal(self.data(), self.host[0])
        return enc


# ---- known answers -------------------------------------------------------------------------------------------------------------

def test_known_answer_at_an_odd_address(ctx):
    n, off, size, first, sub = layout([[(0, 64)]], [47], lead=49)
    data = np.full(n, CAN, dtype=np.uint8)
    data[49:113] = np.frombuffer(PLAIN_38A, dtype=np.uint8)
    c = Crypt(data, off, size, first, sub, KEY_38A, iv=np.arange(16, dtype=np.uint8), c=1, k=0)
    enc = c.there_and_back(ctx)
    assert bytes(enc[49:113]) == CBC_38A and (enc[:49] == CAN).all() and (enc[113:] == CAN).all()
    want, done = R.crypt(data, off, size, first, sub, KEY_38A, iv0=bytes(range(16)), c=1, k=0)          # the sequential reference says the same
    assert done == 64 and np.array_equal(want, enc)


# ---- pattern edges --------------------------------------------------------------------------------------------------------------

def edge_case(c, k, seed):
    rng = np.random.default_rng(seed)
    period = sum(R.pattern(c, k))
    protects = sorted({0, 1, 15, 16, 17} | {16 * nb + t for nb in range(2 * period + 2) for t in (0, 7)})
    entries, cur = [], []
    for p in protects:                                      # each protect twice, in samples of one to four entries
        for _ in range(2):
            cur.append((int(rng.integers(0, 21)), p))
            if len(cur) == 1 + len(entries) % 4:
                entries.append(cur)
                cur = []
    entries.append(cur)
    n, off, size, first, sub = layout(entries, rng.integers(0, 20, len(entries)).tolist(), lead=int(rng.integers(1, 16)))
    return rng.integers(0, 256, n, dtype=np.uint8), off, size, first, sub, rng


@pytest.mark.parametrize("decrypt", (False, True), ids=("encrypt", "decrypt"))
@pytest.mark.parametrize("whole", (False, True), ids=("partial", "whole"))
@pytest.mark.parametrize("c,k", PATTERNS)
def test_pattern_edges(ctx, c, k, whole, decrypt):
    data, off, size, first, sub, rng = edge_case(c, k, 300 + 16 * c + k)
    x = Crypt(data, off, size, first, sub, bytes(rng.integers(0, 256, 16, dtype=np.uint8)), iv=rng.integers(0, 256, 16 * len(off), dtype=np.uint8),
              c=c, k=k, whole=whole, decrypt=decrypt)
    assert x.launch(ctx) == 0
    got = x.check(ctx)
    # by hand: the bytes that changed lie in crypt blocks, and the count is the closed form's
    inside = np.zeros(len(data), dtype=bool)
    for s in range(len(off)):
        p = int(off[s])
        for clear, protect in sub[int(first[s]):int(first[s + 1])].tolist():
            p += clear
            for i in R.crypt_block_list(c, k, whole, protect // 16):
                inside[p + 16 * i: p + 16 * i + 16] = True
            p += protect
    assert np.array_equal(got[~inside], data[~inside]) and inside.sum() == int(ctx.read_summary(x.summary)["rbsp_bytes"]) > 0


@pytest.mark.parametrize("shift", range(16))
def test_first_crypt_block_at_every_shift(ctx, shift):
    """a short entry and one of 70 crypt blocks (a wavefront's, when decrypting) whose first blocks lie at 32 + shift and behind"""
    rng = np.random.default_rng(500 + shift)
    for c, k in ((1, 0), (1, 9)):
        n, off, size, first, sub = layout([[(0, 16 * 5 + 3), (5, 16 * (70 if k == 0 else 691) + 9)]], [40], lead=32 + shift)
        data = rng.integers(0, 256, n, dtype=np.uint8)
        x = Crypt(data, off, size, first, sub, bytes(rng.integers(0, 256, 16, dtype=np.uint8)), iv=rng.integers(0, 256, 16, dtype=np.uint8), c=c, k=k)
        enc = x.there_and_back(ctx)
        assert int(ctx.read_summary(x.summary)["rbsp_bytes"]) == 16 * ((5 + 70) if k == 0 else (1 + 70))
        assert np.array_equal(enc[: 32 + shift], data[: 32 + shift]) and not np.array_equal(enc[32 + shift: 48 + shift], data[32 + shift: 48 + shift])


# ---- restart per entry, IV modes ---------------------------------------------------------------------------------------------------

def test_chain_and_pattern_restart_at_every_entry(ctx):
    rng = np.random.default_rng(41)
    body = rng.integers(0, 256, 7 + 16 * 23 + 4, dtype=np.uint8)
    filler = [(65535, 0)] * 3
    n, off, size, first, sub = layout([[(7, len(body) - 7)] * 2, filler + [(9, 330)], [(65535, 0), (65535, 0)], [(0, 48)]], [3, 0, 5, 9], lead=11)
    data = rng.integers(0, 256, n, dtype=np.uint8)
    data[11: 11 + len(body)] = body
    data[11 + len(body): 11 + 2 * len(body)] = body
    for c, k in ((1, 9), (3, 7), (1, 0)):
        x = Crypt(data, off, size, first, sub, bytes(range(16)), iv=rng.integers(0, 256, 16 * 4, dtype=np.uint8), c=c, k=k)
        enc = x.there_and_back(ctx)
        a, b = enc[11: 11 + len(body)], enc[11 + len(body): 11 + 2 * len(body)]
        assert np.array_equal(a, b) and not np.array_equal(a, body) and np.array_equal(a[:7], body[:7])
        # the protected entry behind three fillers: its first crypt block is at 3 x 65535 + 9 of the sample
        p = int(off[1]) + 3 * 65535 + 9
        assert np.array_equal(enc[int(off[1]): p], data[int(off[1]): p]) and not np.array_equal(enc[p: p + 16], data[p: p + 16])


def test_both_iv_modes(ctx):
    import torch
    rng = np.random.default_rng(77)
    n, off, size, first, sub = layout([[(3, 40)], [(0, 17), (5, 0)], [(1, 333)], [], [(2, 64)]], [5, 0, 9, 3, 11], lead=7)
    data = rng.integers(0, 256, n, dtype=np.uint8)
    key, iv0 = bytes(range(16)), bytes(rng.integers(0, 256, 16, dtype=np.uint8))
    outs = []
    for iv in ("own", None):                                # a poisoned d_iv (0xC3 bytes), and none: iv0 for every sample
        x = Crypt(data, off, size, first, sub, key, iv0=iv0, c=1, k=0)
        assert x.launch(ctx, iv=iv) == 0
        outs.append(x.check(ctx))
        assert (x.d_iv.cpu().numpy() == CAN).all()
    assert np.array_equal(outs[0], outs[1])
    # iv_mode 0 with iv0 in every row is the same; with other rows it is not
    same = Crypt(data, off, size, first, sub, key, iv=np.tile(np.frombuffer(iv0, dtype=np.uint8), 5), c=1, k=0)
    assert same.launch(ctx) == 0
    assert np.array_equal(same.check(ctx), outs[0])
    other = Crypt(data, off, size, first, sub, key, iv=rng.integers(0, 256, 16 * 5, dtype=np.uint8), c=1, k=0)
    enc = other.there_and_back(ctx)
    assert not np.array_equal(enc, outs[0])
    odd = torch.zeros(16 * 5 + 16, dtype=torch.uint8, device="cuda")[1:]
    assert other.launch(ctx, iv=odd) == R.E_ARG


# ---- the lane / wavefront threshold --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c,k", ((1, 9), (1, 0)))
def test_around_the_lane_wavefront_threshold(ctx, c, k):
    rng = np.random.default_rng(900 + k)
    counts = (1, 63, 64, 65, 127, 128, 129, 4097)
    assert LANE_BLOCKS in counts
    entries = [[(int(rng.integers(0, 30)), 16 * ((m - 1) * (c + k) + 1) + int(rng.integers(0, 16)))] for m in counts]
    n, off, size, first, sub = layout(entries, rng.integers(1, 40, len(entries)).tolist(), lead=5)
    assert [R.crypt_blocks(c, k, False, int(p) // 16) for p in sub["protect"]] == list(counts)
    data = rng.integers(0, 256, n, dtype=np.uint8)
    x = Crypt(data, off, size, first, sub, bytes(rng.integers(0, 256, 16, dtype=np.uint8)), iv=rng.integers(0, 256, 16 * len(off), dtype=np.uint8), c=c, k=k)
    enc, done = x.want()                                    # the reference's ciphertext, once
    assert done == 16 * sum(counts)
    assert x.launch(ctx) == 0                               # encrypt on the device: the reference's bytes
    x.check(ctx, want=(enc, done))
    y = Crypt(enc, off, size, first, sub, x.key, iv=x.iv, c=c, k=k, decrypt=True)      # decrypt on the device of the reference's ciphertext
    assert y.launch(ctx) == 0
    y.check(ctx)
    assert np.array_equal(y.data(), data)


# ---- scale -------------------------------------------------------------------------------------------------------------------------

def scale_case():
    rng = np.random.default_rng(4343)
    E = RANGES * 256 + 1000                                 # at least one range takes two steps of 256
    clear, protect = rng.integers(0, 21, E), rng.integers(16, 49, E)
    per = rng.integers(0, 7, E)                             # entries a sample, until they are used up
    ends = np.cumsum(per)
    ns = int(np.searchsorted(ends, E)) + 1
    first = np.concatenate([[0], np.minimum(ends[:ns], E)]).astype(np.uint64)
    first[-1] = E
    total = np.concatenate([[0], np.cumsum(clear + protect)])
    size = (total[first[1:].astype(np.int64)] - total[first[:-1].astype(np.int64)]).astype(np.uint64)
    gaps = rng.integers(0, 9, ns)
    off = (3 + np.concatenate([[0], np.cumsum(size.astype(np.int64) + gaps)[:-1]])).astype(np.uint64)
    sub = np.zeros(E, dtype=R.SUBSAMPLE)
    sub["clear"], sub["protect"] = clear, protect
    n = int(off[-1] + size[-1]) + 21
    return n, off, size, first, sub, rng


def test_scale_more_entries_than_one_step_a_range(ctx):
    n, off, size, first, sub, rng = scale_case()
    assert len(sub) == RANGES * 256 + 1000 and 9_000_000 < n < 13_000_000
    data = rng.integers(0, 256, n, dtype=np.uint8)
    x = Crypt(data, off, size, first, sub, bytes(rng.integers(0, 256, 16, dtype=np.uint8)), iv=rng.integers(0, 256, 16 * len(off), dtype=np.uint8), c=1, k=0)
    enc = x.there_and_back(ctx)
    assert not np.array_equal(enc, data)


# ---- offsets above 2^32 -------------------------------------------------------------------------------------------------------------

def test_samples_around_offset_4gib(ctx):
    import torch
    rng = np.random.default_rng(4096)
    G, total = 1 << 32, (1 << 32) + (64 << 20)
    big = torch.empty(total, dtype=torch.uint8, device="cuda")
    # windows of the buffer that are written and compared; samples (window, offset in it, entries)
    windows = [(0, 4096), (G - 8192, 16384), (total - 4096, 4096)]
    placed = [(0, 100, [(9, 16 * 21 + 5)]), (1, 1000, [(3, 160), (0, 75)]), (1, 8192 - 1500, [(11, 16 * 180 + 2)]),      # the third lies across 2^32
              (1, 8192 + 1500, [(0, 16 * 70)]), (1, 8192 + 3000, [(65535 - 65530, 33)]), (2, 4096 - 16 * 30 - 7, [(7, 16 * 30)])]
    off = np.array([windows[w][0] + o for w, o, _ in placed], dtype=np.uint64)
    _, _, size, first, sub = layout([e for _, _, e in placed], [0] * len(placed))
    assert int(off[2]) < G < int(off[2] + size[2]) and int(off[-1] + size[-1]) == total
    host = [rng.integers(0, 256, z, dtype=np.uint8) for _, z in windows]
    plain = host
    for (lo, z), h in zip(windows, host):
        big[lo: lo + z] = torch.from_numpy(h).cuda()
    key, iv = bytes(rng.integers(0, 256, 16, dtype=np.uint8)), rng.integers(0, 256, 16 * len(off), dtype=np.uint8)
    d_off, d_size, d_first, d_sub, d_iv = dev(off), dev(size), dev(first), dev(sub), dev(iv)
    import hevcbitstream_amd as hbs
    for decrypt in (False, True):
        want = []
        for w, (lo, z) in enumerate(windows):               # the reference, window by window, on offsets rebased to the window
            mine = [i for i, (pw, _, _) in enumerate(placed) if pw == w]
            _, _, wsize, wfirst, wsub = layout([placed[i][2] for i in mine], [0] * len(mine))
            woff = np.array([placed[i][1] for i in mine], dtype=np.uint64)
            out, done = R.crypt_many(host[w], woff, wsize, wfirst, wsub, key, iv=np.concatenate([iv[16 * i: 16 * i + 16] for i in mine]), c=1, k=0,
                                     decrypt=decrypt)
            want.append((out, done))
        summary = fresh_summary()
        prm = hbs.cbcs_params(key, flags=hbs.CBCS_DECRYPT if decrypt else 0, crypt_byte_block=1, skip_byte_block=0)
        assert ctx.cbcs_crypt_async(big, total, d_off, d_size, len(off), d_first, d_sub, d_iv, prm, summary) == 0
        assert summary_dict(ctx.read_summary(summary)) == dict(error=0, nal_count=len(sub), nal_found=len(off), rbsp_bytes=sum(d for _, d in want),
                                                               stream_bytes=total, stop_reason=0, reserved=[0, 0, 0])
        for (lo, z), (out, _) in zip(windows, want):
            got = big[lo: lo + z].cpu().numpy()
            assert np.array_equal(got, out), (lo, np.flatnonzero(got != out)[:8])
        if not decrypt:
            assert not np.array_equal(want[1][0], host[1])
            host = [out for out, _ in want]
    assert all(np.array_equal(out, p) for (out, _), p in zip(want, plain))              # the second call restored the windows


# ---- each error alone, refusals ------------------------------------------------------------------------------------------------------

def error_base():
    rng = np.random.default_rng(31)
    entries = [[(int(rng.integers(0, 20)), int(rng.integers(1, 50))) for _ in range(int(rng.integers(1, 5)))] for _ in range(600)]
    n, off, size, first, sub = layout(entries, rng.integers(1, 9, 600).tolist(), lead=3)
    return dict(data=rng.integers(0, 256, n, dtype=np.uint8), off=off, size=size, first=first, sub=sub, key=bytes(range(16)),
                iv=rng.integers(0, 256, 16 * 600, dtype=np.uint8), c=1, k=0)


@pytest.mark.parametrize("decrypt", (False, True), ids=("encrypt", "decrypt"))
@pytest.mark.parametrize("what", ("short", "overlap", "past", "clear", "first"))
def test_each_error_alone(ctx, what, decrypt):
    b = error_base()
    j = 311
    if what == "short":
        b["size"][j] += 1                                   # (the gap behind it is at least one byte)
    elif what == "overlap":
        b["off"][j + 1] = b["off"][j] + b["size"][j] - np.uint64(1)
    elif what == "past":
        j = 599
        b["data"] = b["data"][: int(b["off"][j] + b["size"][j]) - 1]
    elif what == "clear":
        e = int(b["first"][j])
        b["size"][j] += np.uint64(65536 - int(b["sub"]["clear"][e]))
        b["off"][j + 1:] += np.uint64(65536)
        b["data"] = np.concatenate([b["data"], np.zeros(65536, dtype=np.uint8)])
        b["sub"]["clear"][e] = 65536
    else:
        b["first"][j + 1] = b["first"][j] - np.uint64(1)      # d_sub_first falls
    assert R.crypt_check(len(b["data"]), b["off"], b["size"], b["first"], b["sub"]) == j + 1
    c = Crypt(decrypt=decrypt, **b)
    assert c.launch(ctx) == 0
    assert summary_dict(ctx.read_summary(c.summary)) == dict(error=R.E_ARG, nal_count=0, nal_found=600, rbsp_bytes=0, stream_bytes=len(b["data"]),
                                                             stop_reason=0, reserved=[j + 1, 0, 0])
    assert np.array_equal(c.data(), b["data"])


def test_refused_at_once_and_no_samples(ctx):
    import torch
    import hevcbitstream_amd as hbs
    b = error_base()
    x = Crypt(**b)
    n = len(b["data"])
    odd = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")

    def call(**change):
        """the C call itself with one argument changed: pointers as integers (None: NULL), params as a record or None"""
        a = dict(data=x.d_data.data_ptr(), data_bytes=n, off=x.d_off.data_ptr(), size=x.d_size.data_ptr(), n_samples=x.n, first=x.d_first.data_ptr(),
                 sub=x.d_sub.data_ptr(), iv=x.d_iv.data_ptr(), params=hbs.cbcs_params(b["key"], crypt_byte_block=1, skip_byte_block=0),
                 summary=x.summary.data_ptr())
        a.update(change)
        prm = a["params"]
        vp = lambda v: None if v is None else C.c_void_p(v)      # noqa: E731
        return ctx.lib.hbs_cbcs_crypt(ctx.h, vp(a["data"]), a["data_bytes"], vp(a["off"]), vp(a["size"]), a["n_samples"], vp(a["first"]), vp(a["sub"]),
                                      vp(a["iv"]), None if prm is None else prm.ctypes.data_as(C.c_void_p), vp(a["summary"]))

    def params(**fields):
        p = hbs.cbcs_params(b["key"], crypt_byte_block=1, skip_byte_block=0)
        for name, v in fields.items():
            p[name] = v
        return p

    refused = [dict(params=None), dict(params=params(iv_mode=2)), dict(params=params(flags=4)), dict(params=params(flags=0x80000001)),
               dict(params=params(crypt_byte_block=16)), dict(params=params(skip_byte_block=16)), dict(params=params(crypt_byte_block=0, skip_byte_block=1)),
               dict(params=params(reserved0=1)), dict(params=params(reserved1=1)), dict(iv=None), dict(n_samples=1 << 32),
               dict(off=None), dict(size=None), dict(first=None), dict(sub=None), dict(data=None), dict(summary=None),
               dict(data=odd.data_ptr() + 1), dict(iv=odd.data_ptr() + 8), dict(summary=odd.data_ptr() + 8),
               dict(off=x.d_off.data_ptr() + 4), dict(size=x.d_size.data_ptr() + 4), dict(first=x.d_first.data_ptr() + 4), dict(sub=x.d_sub.data_ptr() + 4)]
    for change in refused:
        assert call(**change) == R.E_ARG, change
    torch.cuda.synchronize()
    assert (x.summary.cpu().numpy() == 0x5A).all() and np.array_equal(x.data(), b["data"]) and (odd.cpu().numpy() == 0).all()
    assert call() == 0                                      # ... and unchanged it is accepted
    x.check(ctx)
    # iv_mode 1 needs no d_iv; no samples is valid and needs no tables
    e = Crypt(b["data"], b["off"][:0], b["size"][:0], b["first"][:1], b["sub"][:0], b["key"], iv0=bytes(16))
    assert e.launch(ctx, iv=None) == 0
    assert summary_dict(ctx.read_summary(e.summary)) == dict(error=0, nal_count=0, nal_found=0, rbsp_bytes=0, stream_bytes=n, stop_reason=0,
                                                             reserved=[0, 0, 0])
    assert np.array_equal(e.data(), b["data"])


# ---- HIP graphs ----------------------------------------------------------------------------------------------------------------

def replay(launch, load, check, ctx):
    """captured on a side stream after one warm-up call on contents 0, replayed on contents 1 and 0 of the same buffers"""
    import torch
    side = torch.cuda.Stream()
    load(0)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert launch() == 0
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            launch()
    check(0)
    held = ctx.device_bytes()
    for which in (1, 0):
        load(which)
        g.replay()
        torch.cuda.synchronize()
        check(which)
    assert ctx.device_bytes() == held


@pytest.mark.parametrize("decrypt", (False, True), ids=("encrypt", "decrypt"))
def test_one_replay_from_a_graph(ctx, decrypt):
    import torch
    rng = np.random.default_rng(808)
    shapes = []
    for _ in range(2):                                      # two tables of 300 samples and 900 entries over one buffer size
        entries = [[(int(rng.integers(0, 30)), int(rng.integers(0, 300))) for _ in range(2)] + [(5, 16 * int(rng.integers(60, 70)))] for _ in range(300)]
        shapes.append(layout(entries, [0] * 300, lead=int(rng.integers(0, 16))))
    n = max(s[0] for s in shapes) + 16
    datas = [rng.integers(0, 256, n, dtype=np.uint8) for _ in range(2)]
    ivs = [rng.integers(0, 256, 16 * 300, dtype=np.uint8) for _ in range(2)]
    key = bytes(rng.integers(0, 256, 16, dtype=np.uint8))
    c = Crypt(datas[0], *shapes[0][1:], key, iv=ivs[0], c=1, k=0, decrypt=decrypt)

    def load(i):
        for t, a in zip((c.d_data, c.d_off, c.d_size, c.d_first, c.d_sub, c.d_iv), (datas[i],) + shapes[i][1:] + (ivs[i],)):
            t.copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()))
        c.summary.fill_(0x5A)

    def check(i):
        want, done = R.crypt_many(datas[i], *shapes[i][1:], key, iv=ivs[i], c=1, k=0, decrypt=decrypt)
        s = summary_dict(ctx.read_summary(c.summary))
        assert s["rbsp_bytes"] == done and s["error"] == 0 and s["nal_count"] == 900
        assert np.array_equal(c.data(), want)
    replay(lambda: c.launch(ctx), load, check, ctx)


# ---- end to end ----------------------------------------------------------------------------------------------------------------

def test_end_to_end_on_a_live_context(ctx):
    """fragment, subsample table, cbcs encrypt, hbs_cenc_crypt on another buffer in between (the two share their scratch), cbcs decrypt"""
    import torch
    import hevcbitstream_amd as hbs
    from hevcbitstream_amd.api import COMPACT, PARSED, SUMMARY
    from tests import _cenc_ref as RC
    from tests.hevc_synth import stream_4k30
    stream, n = stream_4k30(9, n_pictures=36, slices_per_picture=2, idr_every=12, payload_bytes=(60, 400))
    d = torch.from_numpy(np.frombuffer(stream, dtype=np.uint8).copy()).cuda()
    cap = n + 8
    index, parsed, cc = (torch.zeros(cap * z, dtype=torch.uint8, device="cuda") for z in (32, PARSED.itemsize, COMPACT.itemsize))
    structs = torch.zeros(8 << 20, dtype=torch.uint8, device="cuda")
    po = torch.zeros(cap * 8, dtype=torch.uint8, device="cuda")
    ss, ps = (torch.zeros(SUMMARY.itemsize, dtype=torch.uint8, device="cuda") for _ in range(2))
    got = ctx.index_parse_compact_async(d, index, cap, parsed, cc, structs, ss, ps, payload_off=po)
    assert got == n and int(ctx.read_summary(ps)["error"]) == 0
    au, nal_au, s, _ = ctx.access_units(index, parsed, cc, structs, got)
    n_aus = len(au)
    idx = index[: got * 32]
    out, so, sz, frags, _ = ctx.mp4_fragment(d, idx, nal_au, au, flags=hbs.MP4_CUT_AT_IRAP, sample_duration=3003, track_id=1)
    assert len(frags) == 3
    plain = out.cpu().numpy().copy()
    sub_first, sub, s = ctx.cenc_subsamples(d, idx, nal_au, n_aus, payload_off=po[: got * 8], length_size=4)
    h_first, h_sub = sub_first.cpu().numpy().view(np.uint64), sub.cpu().numpy().view(R.SUBSAMPLE)
    assert int(s["stream_bytes"]) == int(sz.sum()) and int(h_sub["protect"].max()) >= 16 * 11
    key, iv0 = bytes(range(16, 32)), bytes(range(100, 116))
    s = ctx.cbcs_crypt(out, so, sz, sub_first, sub, key, iv0=iv0)                       # 1:9, the constant IV
    want, done = R.crypt_many(plain, so, sz, h_first, h_sub, key, iv0=iv0)
    enc = out.cpu().numpy()
    assert int(s["rbsp_bytes"]) == done > 16 * 36 and int(s["nal_count"]) == len(h_sub) and np.array_equal(enc, want)
    assert (enc != plain).sum() <= done and not np.array_equal(enc, plain)
    # hbs_cenc_crypt on a copy of the fragments, on the same context
    other = torch.from_numpy(plain.copy()).cuda()
    ctx.cenc_crypt(other, so, sz, sub_first, sub, key, iv0=bytes(8))
    assert np.array_equal(other.cpu().numpy(), RC.crypt(plain, so, sz, h_first, h_sub, key, iv0=bytes(8))[0])
    assert np.array_equal(out.cpu().numpy(), enc)
    # and back
    s = ctx.cbcs_crypt(out, so, sz, sub_first, sub, key, iv0=iv0, decrypt=True)
    assert int(s["rbsp_bytes"]) == done and np.array_equal(out.cpu().numpy(), plain)
    h_idx = idx.cpu().numpy().view(NAL_ENTRY)
    src = np.frombuffer(stream, dtype=np.uint8)
    back, _, _ = ctx.lenpref_to_annexb(out, so, sz, length_size=4, startcode_bytes=4)
    assert bytes(back.cpu().numpy()) == b"".join(b"\x00\x00\x00\x01" + bytes(src[int(e["start"]):int(e["end"])]) for e in h_idx)


# ---- many long entries in a step, decrypting ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("c,k", ((1, 0), (1, 9)))
def test_many_long_entries_in_a_step(ctx, c, k):
    """the large tables of tests/_seq_cases.py: 2 to 15 entries of kCbcsLaneBlocks crypt blocks and more in every range, more than
    four in nine ranges of ten (tests/test_seq_cases.py), so the decrypting kernel lists more entries in a step than it has
    wavefronts.  Random bytes are the ciphertext.  With 1:9 the long entries are scaled to the same 64 to 70 crypt blocks.  Then
    the device's encryption of the device's plaintext, against the reference on the same tables (all samples: the reference's step
    loop has the 70 steps of the longest chain whatever the pattern, under two seconds), gives the ciphertext back"""
    from tests import _seq_cases as S
    t = S.crypt_tables("large", 1)
    rng = np.random.default_rng(1700 + k)
    sub, first = t["sub"].copy(), t["first"]
    if k:                                                   # m crypt blocks of 1:9 are (m - 1) x 10 + 1 blocks
        long_ = sub["protect"] // 16 >= LANE_BLOCKS
        sub["protect"][long_] = 16 * ((sub["protect"][long_] // 16 - 1) * (c + k) + 1) + sub["protect"][long_] % 16
    blocks = np.array([R.crypt_blocks(c, k, False, int(p) // 16) for p in sub["protect"]])
    begin = [S.crypt_entries(t) // RANGES * g + S.crypt_entries(t) % RANGES * g // RANGES for g in range(RANGES + 1)]
    listed = np.diff(np.concatenate([[0], np.cumsum(blocks >= LANE_BLOCKS)])[begin])
    assert (listed > 4).sum() >= 900 and listed.min() >= 1 and max(np.diff(begin)) <= 256 and blocks.max() <= 70
    total = np.concatenate([[0], np.cumsum(sub["clear"].astype(np.int64) + sub["protect"])])
    size = (total[first[1:].astype(np.int64)] - total[first[:-1].astype(np.int64)]).astype(np.uint64)
    off = (3 + np.concatenate([[0], np.cumsum(size.astype(np.int64) + 5)[:-1]])).astype(np.uint64)
    n = int(off[-1] + size[-1]) + 11
    cipher = rng.integers(0, 256, n, dtype=np.uint8)
    x = Crypt(cipher, off, size, first, sub, bytes(rng.integers(0, 256, 16, dtype=np.uint8)), iv=rng.integers(0, 256, 16 * len(off), dtype=np.uint8), c=c, k=k,
              decrypt=True)
    assert x.launch(ctx) == 0
    plain = x.check(ctx)
    assert int(ctx.read_summary(x.summary)["rbsp_bytes"]) == 16 * int(blocks.sum())
    x.direction(False)
    assert x.launch(ctx) == 0
    back = x.check(ctx, before=plain)
    assert np.array_equal(back, cipher)


# ---- carved buffers ----------------------------------------------------------------------------------------------------------------

def test_carved_buffers_at_each_accepted_alignment(ctx):
    """every pointer of the call inside a larger allocation, at each offset from a page boundary its alignment accepts -- each goes
    through its whole set while the others rotate; 4 KiB of known bytes lie on both sides of every buffer and are looked at
    afterwards.  data_bytes is no multiple of 16 and the last sample ends on the last byte"""
    import hevcbitstream_amd as hbs
    rng = np.random.default_rng(66)
    for j in range(len(K.OFFS8)):
        o16 = lambda i: K.OFFS16[(j + i) % len(K.OFFS16)]          # noqa: E731
        o8 = lambda i: K.OFFS8[(j + i) % len(K.OFFS8)]             # noqa: E731
        entries = [[(int(rng.integers(0, 21)), int(rng.integers(0, 400))) for _ in range(int(rng.integers(0, 5)))] for _ in range(39)]
        entries.append([(4, 16 * 70 + 9)])                  # a wavefront's entry, when decrypting, up to the buffer's last bytes
        lead = int(rng.integers(0, 16))
        n, off, size, first, sub = layout(entries, rng.integers(0, 9, 39).tolist() + [0], lead=lead)
        if n % 16 == 0:
            n, off, size, first, sub = layout(entries, rng.integers(0, 9, 39).tolist() + [0], lead=lead + 1)
        assert n % 16 and int(off[-1] + size[-1]) == n
        c, k = PATTERNS[j % len(PATTERNS)]
        decrypt, whole, const = bool(j % 2), bool(j % 3 == 0), j % 4 == 3
        data, key, ns = rng.integers(0, 256, n, dtype=np.uint8), bytes(rng.integers(0, 256, 16, dtype=np.uint8)), len(off)
        iv, iv0 = rng.integers(0, 256, 16 * ns, dtype=np.uint8), bytes(rng.integers(0, 256, 16, dtype=np.uint8))
        want, done = R.crypt_many(data, off, size, first, sub, key, iv=None if const else iv, iv0=iv0 if const else None, c=c, k=k, whole=whole, decrypt=decrypt)
        cd = K.Carved(n, o16(0), CAN, K.PAD, True).put(data)
        co = K.Carved(ns * 8, o8(1), 0xFF, K.PAD, True).put(off)
        cz = K.Carved(ns * 8, o8(4), 0xFF, K.PAD, True).put(size)
        cf = K.Carved((ns + 1) * 8, o8(7), 0xFF, K.PAD, True).put(first)
        cs = K.Carved(len(sub) * 8, o8(9), 0xFF, K.PAD, True).put(sub)
        ci = K.Carved(ns * 16, o16(3), CAN, K.PAD, True).put(iv)
        cm = K.Carved(64, o16(5), 0xEE, K.PAD, True)
        prm = hbs.cbcs_params(key, iv0=iv0 if const else None, flags=(hbs.CBCS_DECRYPT if decrypt else 0) | (hbs.CBCS_WHOLE_RUNS if whole else 0),
                              crypt_byte_block=c, skip_byte_block=k)
        assert ctx.cbcs_crypt_async(cd.view, n, co.view, cz.view, ns, cf.view, cs.view, ci.view, prm, cm.view) == 0, j
        summary_matches(ctx.read_summary(cm.view), dict(error=0, nal_count=len(sub), nal_found=ns, rbsp_bytes=done, stream_bytes=n, stop_reason=0,
                                                        reserved=[0, 0, 0]))
        assert np.array_equal(cd.get(), want) and np.array_equal(ci.get(), iv), j
        for name, cv in (("data", cd), ("sample_off", co), ("sample_size", cz), ("sub_first", cf), ("sub", cs), ("iv", ci), ("summary", cm)):
            assert cv.intact(), (j, name, cv.damage())
