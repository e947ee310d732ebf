"""Buffers carved out of larger allocations (test infrastructure; not a conftest, no fixtures).

Every other test hands the library torch allocations: aligned to 256 bytes or more, each at the start of its own block, with
allocator leftovers around it.  carve() puts a buffer at a chosen offset from a 4096-byte boundary, in the middle of one
allocation whose other bytes are known, so that
  - a pointer that is 16-byte but not 64 / 256 / 1024 / 4096-byte aligned reaches the kernels,
  - a store in front of or behind an output lands in bytes that are looked at afterwards,
  - whatever a kernel reads outside an input is chosen by the test (hostile()).
No buffer lies against an end of its allocation: an access outside one is found by value, never by a fault.

carve() works on the GPU (torch uint8 tensors); carve_host() does the same over numpy arrays for the CPU single-stepper."""
import numpy as np

PAD = 4096
FILL = 0xC3
PAGE = 4096


def _pattern(fill, n):
    if isinstance(fill, (int, np.integer)):
        return np.full(n, int(fill), dtype=np.uint8)
    p = np.frombuffer(bytes(fill), dtype=np.uint8)
    assert len(p) > 0
    return np.tile(p, n // len(p) + 1)[:n].copy()


class Carved:
    """one carved buffer: .view (the tensor / array handed to the call), .ptr, .offset, and the padding's check"""

    def __init__(self, nbytes, offset, fill, pad, on_gpu):
        assert pad >= PAD and offset >= 0 and nbytes >= 0
        self.nbytes, self.offset, self.pad, self.on_gpu = int(nbytes), int(offset), int(pad), on_gpu
        total = 2 * self.pad + self.offset + self.nbytes
        self.lo = self.pad + self.offset
        self.hi = self.lo + self.nbytes
        self.expect = _pattern(fill, total)                 # what the whole allocation holds outside the view
        if on_gpu:
            import torch
            raw = torch.empty(total + PAGE, dtype=torch.uint8, device="cuda")
            skip = (-raw.data_ptr()) % PAGE
            self.buf = raw[skip: skip + total]
            self.buf.copy_(torch.from_numpy(self.expect))
            self.base = self.buf.data_ptr()
        else:
            raw = np.empty(total + PAGE, dtype=np.uint8)
            skip = (-raw.ctypes.data) % PAGE
            self.buf = raw[skip: skip + total]
            self.buf[:] = self.expect
            self.base = self.buf.ctypes.data
        assert self.base % PAGE == 0, "the allocation's base is not page aligned"
        self.view = self.buf[self.lo: self.hi]
        self.ptr = self.base + self.lo
        assert self.ptr % PAGE == self.offset % PAGE
        if on_gpu and self.nbytes:
            assert self.view.data_ptr() == self.ptr

    def put(self, data):
        """the view's bytes := data (any numpy array of nbytes bytes)"""
        a = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        assert len(a) == self.nbytes, (len(a), self.nbytes)
        if not self.nbytes:
            return self
        if self.on_gpu:
            import torch
            self.view.copy_(torch.from_numpy(a.copy()))
        else:
            self.view[:] = a
        return self

    def get(self):
        """a host copy of the view's bytes"""
        return self.view.cpu().numpy() if self.on_gpu else self.view.copy()

    def hostile(self, front=b"", back=b""):
        """lay `front` so that it ends right in front of the view and `back` so that it begins right behind it"""
        for at, pat in ((self.lo - len(front), front), (self.hi, back)):
            if len(pat):
                p = np.frombuffer(bytes(pat), dtype=np.uint8)
                assert len(p) <= self.pad
                self.expect[at: at + len(p)] = p
                if self.on_gpu:
                    import torch
                    self.buf[at: at + len(p)].copy_(torch.from_numpy(p.copy()))
                else:
                    self.buf[at: at + len(p)] = p
        return self

    def _sides(self):
        if self.on_gpu:
            return self.buf[: self.lo].cpu().numpy(), self.buf[self.hi:].cpu().numpy()
        return self.buf[: self.lo], self.buf[self.hi:]

    def damage(self):
        """'' when every byte in front of and behind the view holds what was put there, else where the first and last changed
        bytes lie, relative to the view"""
        front, back = self._sides()
        out = []
        bad = np.flatnonzero(front != self.expect[: self.lo])
        if len(bad):
            out.append("%d bytes changed in front of the buffer, %d..%d bytes before its start" % (len(bad), self.lo - int(bad[0]), self.lo - int(bad[-1])))
        bad = np.flatnonzero(back != self.expect[self.hi:])
        if len(bad):
            out.append("%d bytes changed behind the buffer, %d..%d bytes past its end" % (len(bad), int(bad[0]), int(bad[-1])))
        return "; ".join(out)

    def intact(self):
        return self.damage() == ""

    __call__ = intact


def carve(nbytes, offset, fill=FILL, pad=PAD):
    """One uint8 CUDA tensor of pad + offset + nbytes + pad bytes on a 4096-byte boundary, filled with `fill` (a byte or a
    pattern of bytes).  Returns (view, checker): view = [pad + offset, pad + offset + nbytes) of it, so that
    view.data_ptr() % 4096 == offset % 4096; checker() is True while every byte around the view holds the fill (checker.damage()
    says where it does not; checker.put / get / hostile move bytes)."""
    c = Carved(nbytes, offset, fill, pad, True)
    return c.view, c


def carve_host(nbytes, offset, fill=FILL, pad=PAD):
    """carve() over a numpy array: for code that runs on the CPU and takes raw pointers (checker.ptr)"""
    c = Carved(nbytes, offset, fill, pad, False)
    return c.view, c


def hostile(checker, front=b"", back=b""):
    """bytes a kernel must not let into its result, immediately in front of and behind an input view"""
    return checker.hostile(front, back)


# what the issue of this module asks to put around a stream / an arena
STREAM_FRONTS = (b"\x00\x00", b"\x00\x00\x00", b"\x00\x00\x01", b"\x00\x00\x03")
STREAM_BACKS = (b"\x01", b"\x00\x01", b"\x03", b"\x00\x00\x01\x42", b"\x00" * 64, b"\xff" * 64)      # the last one is the control

# offsets from a 4096-byte boundary: a line, 256 B, a 1 KiB row and a page
OFFS16 = (0, 16, 32, 48, 80, 240, 1008, 4080)
OFFS8 = OFFS16 + (8, 24, 56)
OFFS4 = OFFS8 + (4, 12, 60)
OFFS1 = tuple(sorted(set(OFFS16) | set(range(16))))


# ---- streams whose first and last bytes, and the bytes around them, decide a NAL ----------------------------------------------

STREAM_BEGINS = (b"\x01", b"\x00\x01", b"\x00\x00\x01", b"\x03")
STREAM_ENDS = (b"\x55", b"\x00", b"\x00\x00", b"\x00\x00\x00", b"\x00\x00\x03", b"\x00\x00\x01",
               b"\x00\x00\x01\x00\x00\x01", b"\x00\x00\x01\x00\x00\x00\x01")          # the last two: an empty last NAL


def body(rng, n):
    """n bytes without zeros but for NALs of 40-300 bytes (start codes of 3 and 4 bytes), a few 00 00 03 and zero pairs"""
    s = rng.integers(4, 256, size=n, dtype=np.uint8)
    at = int(rng.integers(2, 40))
    while at + 8 < n:
        sc = (0, 0, 1, 0x40) if rng.integers(3) else (0, 0, 0, 1)
        s[at:at + 4] = sc
        if rng.integers(4) == 0 and at + 24 < n:
            s[at + 12:at + 16] = (0, 0, 3, int(rng.integers(0, 4)))
        at += int(rng.integers(40, 300))
    return s


def edge_stream(rng, n, begin, end):
    """a stream of n bytes that begins with `begin` and ends with `end`; a payload byte stands between them and the body"""
    assert n >= len(begin) + len(end) + 2
    s = body(rng, n)
    s[: len(begin)] = np.frombuffer(begin, dtype=np.uint8)
    s[len(begin)] = 0x41
    s[n - len(end) - 1] = 0x80
    s[n - len(end):] = np.frombuffer(end, dtype=np.uint8)
    return s


def hostile_cases():
    """[(front, back, begin, end)]: every front with every begin, every back with every end, paired up in 48 cases"""
    fb = [(f, b) for f in STREAM_FRONTS for b in STREAM_BEGINS]
    be = [(b, e) for b in STREAM_BACKS for e in STREAM_ENDS]
    return [(fb[k % len(fb)][0], be[k][0], fb[k % len(fb)][1], be[k][1]) for k in range(len(be))]


def expected_scan(orc, s):
    """What hbs_index_extract must report for the exact-size array s, from the oracle: (entries, arena, stop_reason, nal_found,
    rbsp_bytes; the last two None where the header leaves them open).  A walk the oracle stops at an empty NAL still counts every start code of the stream and every RBSP byte behind
    them (hbs_summary.nal_found): the oracle's walk of the bytes behind the empty NAL's start code added on, the empty NAL
    itself one more NAL of no bytes."""
    idx, arena, why = orc.index_extract(s)
    found, kept = len(idx), len(arena)
    if why == 1:
        p = int(idx["end"][-1]) if len(idx) else 0
        b = bytes(s[p:])
        q = p + b.index(b"\x00\x00\x01") + 3
        if len(s) - q < 4:
            # nothing but the rest of a start code behind the empty NAL: hbs_summary does not say whether that one counts as
            # found; such a stream is judged by everything else (and by the same call on ordinary buffers)
            return idx, arena, why, None, None
        _, _, _, f2, k2 = expected_scan(orc, s[q:])
        found, kept = (None, None) if f2 is None else (found + 1 + f2, kept + k2)
    return idx, arena, why, found, kept
