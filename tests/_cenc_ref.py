"""Reference for hbs_cenc_subsamples and hbs_cenc_crypt (include/hevcbitstream_amd.h): AES-128 by the text of FIPS-197 --
SubBytes, ShiftRows, MixColumns on a 4x4 byte state, the S-box computed from the field inverse -- the counter rule of ISO/IEC
23001-7 `cenc`, and both rules as plain sequential loops.  `keystream` is the same cipher over many counter blocks at once
(numpy, the byte state kept as arrays), for the large cases; tests/test_cenc_ref.py holds the two against each other and
against published vectors."""
import numpy as np

E_ARG, E_CAPACITY = -3, -4
ALIGN16 = 1
SCHEME_CENC = 0x63656E63
MAX_CLEAR = 65535
SUBSAMPLE = np.dtype([("clear", "<u4"), ("protect", "<u4")])
M64 = (1 << 64) - 1


# ---- AES-128 ---------------------------------------------------------------------------------------------------------------------

def _xtime(b):
    b <<= 1
    return (b ^ 0x11B) & 0xFF if b & 0x100 else b


def _gmul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a = _xtime(a)
        b >>= 1
    return r


def _make_sbox():
    box = []
    for x in range(256):
        inv = 0
        if x:
            inv = next(y for y in range(1, 256) if _gmul(x, y) == 1)
        s = inv
        for i in range(1, 5):
            s ^= ((inv << i) | (inv >> (8 - i))) & 0xFF
        box.append(s ^ 0x63)
    return box


SBOX = _make_sbox()
_SBOX_NP = np.array(SBOX, dtype=np.uint8)
_MUL2 = np.array([_xtime(x) for x in range(256)], dtype=np.uint8)


def expand_key(key):
    """the 11 round keys of a 16-byte key, each 16 bytes"""
    w = [list(key[4 * i: 4 * i + 4]) for i in range(4)]
    rcon = 1
    for i in range(4, 44):
        t = list(w[i - 1])
        if i % 4 == 0:
            t = [SBOX[b] for b in t[1:] + t[:1]]
            t[0] ^= rcon
            rcon = _xtime(rcon)
        w.append([a ^ b for a, b in zip(w[i - 4], t)])
    return [bytes(sum(w[4 * r: 4 * r + 4], [])) for r in range(11)]


def encrypt_block(key, block):
    """AES-128 of one 16-byte block; the state is column-major as in FIPS-197: byte 4 c + r is row r, column c"""
    rk = expand_key(key)
    s = [a ^ b for a, b in zip(block, rk[0])]
    for rnd in range(1, 11):
        s = [SBOX[b] for b in s]
        s = [s[4 * ((c + r) % 4) + r] for c in range(4) for r in range(4)]          # ShiftRows: row r moves r columns left
        if rnd < 10:
            m = []
            for c in range(4):
                a = s[4 * c: 4 * c + 4]
                m += [_gmul(a[r], 2) ^ _gmul(a[(r + 1) % 4], 3) ^ a[(r + 2) % 4] ^ a[(r + 3) % 4] for r in range(4)]
            s = m
        s = [a ^ b for a, b in zip(s, rk[rnd])]
    return bytes(s)


def encrypt_blocks(key, blocks):
    """AES-128 of many blocks at once: blocks uint8 [n, 16] -> uint8 [n, 16]"""
    rk = [np.frombuffer(k, dtype=np.uint8) for k in expand_key(key)]
    s = np.asarray(blocks, dtype=np.uint8).reshape(-1, 16) ^ rk[0]
    shift = np.array([4 * ((c + r) % 4) + r for c in range(4) for r in range(4)])
    for rnd in range(1, 11):
        s = _SBOX_NP[s][:, shift]
        if rnd < 10:
            a = s.reshape(-1, 4, 4)                                     # [block, column, row]
            a1, a2, a3 = np.roll(a, -1, axis=2), np.roll(a, -2, axis=2), np.roll(a, -3, axis=2)
            s = (_MUL2[a] ^ _MUL2[a1] ^ a1 ^ a2 ^ a3).reshape(-1, 16)
        s = s ^ rk[rnd]
    return s


def counter_blocks(ctr, n):
    """the n counter blocks from the 16-byte block ctr on: the addition stays in bytes 8..15 and wraps there"""
    ctr = bytes(ctr)
    lo = int.from_bytes(ctr[8:], "big")
    out = np.zeros((n, 16), dtype=np.uint8)
    out[:, :8] = np.frombuffer(ctr[:8], dtype=np.uint8)
    v = (np.arange(n, dtype=np.uint64) + np.uint64(lo)) if n else np.zeros(0, dtype=np.uint64)      # uint64 addition wraps
    out[:, 8:] = v.astype(">u8").view(np.uint8).reshape(n, 8)
    return out


def keystream(key, ctr, nbytes):
    n = (nbytes + 15) // 16
    return encrypt_blocks(key, counter_blocks(ctr, n)).reshape(-1)[:nbytes]


def sample_ctr(s, iv=None, iv0=None):
    """sample s's counter block: iv (n x 16 bytes) or, sequential, from the first 8 bytes of iv0"""
    if iv0 is None:
        return bytes(bytearray(iv[16 * s: 16 * s + 16]))
    return ((int.from_bytes(bytes(iv0)[:8], "big") + s) & M64).to_bytes(8, "big") + bytes(8)


# ---- the subsample rule ------------------------------------------------------------------------------------------------------------

def emit(out, C, P):
    q = max(-(-C // MAX_CLEAR), 1) - 1
    out += [(MAX_CLEAR, 0)] * q
    out.append((C - MAX_CLEAR * q, P))


def sample_subsamples(nals, L, flags=0, clear_lead=96):
    """the entries of one sample.  nals: [(size, type, h)] of its kept NALs in order, h = the clear lead the payload offset
    gives or None"""
    out, C = [], 0
    for size, typ, h in nals:
        if typ >= 32 or size == 0:
            C += L + size
            continue
        if h is None:
            h = min(clear_lead, size)
        P = size - h
        if flags & ALIGN16:
            h += P % 16
            P -= P % 16
        C += L + h
        if P > 0:
            emit(out, C, P)
            C = 0
    if C > 0:
        emit(out, C, 0)
    return out


def subsamples(stream, starts, ends, nal_au, n_aus, L, keep=None, payload_off=None, flags=0, clear_lead=96, sub_cap=None):
    """hbs_cenc_subsamples -> dict(error, bad (1 + the lowest offending NAL), sub_first, sub, protected, sample_bytes, kept)"""
    n = len(starts)
    bad = 0
    prev_end = 0
    for k in range(n):
        wrong = starts[k] > ends[k] or ends[k] > len(stream) or starts[k] < prev_end
        kept = not wrong and (keep is None or keep[k] != 0)
        if kept and (ends[k] - starts[k]) >> (8 * L):
            wrong = True
        if k and ((int(nal_au[k]) - int(nal_au[k - 1])) & 0xFFFFFFFF) > 1:
            wrong = True
        if k == n - 1 and ((int(nal_au[k]) - int(nal_au[0])) & 0xFFFFFFFF) + 1 != n_aus:
            wrong = True
        if kept and not wrong and payload_off is not None and ends[k] > starts[k] and ((stream[starts[k]] >> 1) & 63) < 32:
            po = int(payload_off[k])
            if po == M64 or po < starts[k] + 2 or po > ends[k]:
                wrong = True
        if wrong and not bad:
            bad = k + 1
        prev_end = ends[k]
    if bad:
        return dict(error=E_ARG, bad=bad)
    per_au = [[] for _ in range(n_aus)]
    sample_bytes = kept_n = 0
    for k in range(n):
        if keep is not None and keep[k] == 0:
            continue
        size = int(ends[k] - starts[k])
        typ = (int(stream[starts[k]]) >> 1) & 63 if size else 63
        h = int(payload_off[k]) - int(starts[k]) if (payload_off is not None and typ < 32 and size) else None
        per_au[(int(nal_au[k]) - int(nal_au[0])) & 0xFFFFFFFF].append((size, typ, h))
        sample_bytes += L + size
        kept_n += 1
    sub, first = [], [0]
    for nals in per_au:
        sub += sample_subsamples(nals, L, flags, clear_lead)
        first.append(len(sub))
    r = dict(error=0, bad=0, sub_first=np.array(first, dtype=np.uint64), sub=np.array(sub, dtype=SUBSAMPLE).reshape(-1),
             protected=sum(p for _, p in sub), sample_bytes=sample_bytes, kept=kept_n)
    if sub_cap is not None and sub_cap < len(sub):
        r["error"] = E_CAPACITY
    return r


# ---- hbs_cenc_crypt ---------------------------------------------------------------------------------------------------------------

def crypt_check(data_bytes, off, size, sub_first, sub):
    """1 + the lowest offending sample, 0: none.  Three groups of checks, each over all samples before the next: where the
    samples lie and d_sub_first; then the clear counts; then the sums (the entries are not read through a table that is wrong)"""
    n = len(off)
    for s in range(n):
        o, z = int(off[s]), int(size[s])
        f0, f1 = int(sub_first[s]), int(sub_first[s + 1])
        if o + z > data_bytes or (s + 1 < n and o + z > int(off[s + 1])) or f0 > f1 or (s == 0 and f0 != 0):
            return s + 1
    for s in range(n):
        if bool((sub[int(sub_first[s]): int(sub_first[s + 1])]["clear"] > MAX_CLEAR).any()):
            return s + 1
    for s in range(n):
        e = sub[int(sub_first[s]): int(sub_first[s + 1])]
        if int(e["clear"].astype(np.uint64).sum() + e["protect"].astype(np.uint64).sum()) != int(size[s]):
            return s + 1
    return 0


def crypt(data, off, size, sub_first, sub, key, iv=None, iv0=None):
    """hbs_cenc_crypt on a copy of data (uint8 array) -> (the data behind the call, bytes XORed, the n x 16 counter blocks)"""
    out = np.array(data, dtype=np.uint8, copy=True)
    done = 0
    used = np.zeros((len(off), 16), dtype=np.uint8)
    for s in range(len(off)):
        ctr = sample_ctr(s, iv, iv0)
        used[s] = np.frombuffer(ctr, dtype=np.uint8)
        e = sub[int(sub_first[s]): int(sub_first[s + 1])]
        total = int(e["protect"].astype(np.uint64).sum())
        if not total:
            continue
        ks = keystream(key, ctr, total)
        p, j = int(off[s]), 0
        for clear, protect in zip(e["clear"].tolist(), e["protect"].tolist()):
            p += clear
            out[p: p + protect] ^= ks[j: j + protect]
            p += protect
            j += protect
        done += total
    return out, done, used
