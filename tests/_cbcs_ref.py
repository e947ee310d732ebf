"""Reference for hbs_cbcs_crypt (include/hevcbitstream_amd.h): the inverse cipher of AES-128 by the text of FIPS-197 5.3 --
InvShiftRows, InvSubBytes, InvMixColumns on a 4x4 byte state, the round keys of the cipher in reverse order -- CBC, the block
pattern of ISO/IEC 23001-7 `cbcs`, and `crypt` as one sequential loop per entry.  `crypt_many` is the same over all entries at
once (numpy: the chains side by side, a step of all of them at a time when encrypting, every block at once when decrypting), for
the large cases; tests/test_cbcs_ref.py holds the two against each other and against published vectors.  The forward cipher, the
key expansion and the checks of the samples are tests/_cenc_ref.py's."""
import numpy as np

from tests._cenc_ref import (E_ARG, MAX_CLEAR, SBOX, SUBSAMPLE, _gmul, crypt_check, encrypt_block, encrypt_blocks,  # noqa: F401
                             expand_key)

DECRYPT, WHOLE_RUNS = 1, 2
PARAMS = np.dtype([("key", "u1", (16,)), ("iv0", "u1", (16,)), ("iv_mode", "<u4"), ("flags", "<u4"), ("crypt_byte_block", "u1"),
                   ("skip_byte_block", "u1"), ("reserved0", "<u2"), ("reserved1", "<u4")])

INV_SBOX = [0] * 256
for _x, _s in enumerate(SBOX):
    INV_SBOX[_s] = _x
_INV_NP = np.array(INV_SBOX, dtype=np.uint8)
_MUL = {m: np.array([_gmul(x, m) for x in range(256)], dtype=np.uint8) for m in (9, 11, 13, 14)}
# InvShiftRows: row r moves r columns right; byte 4 c + r is row r, column c
_INV_SHIFT = [4 * ((c - r) % 4) + r for c in range(4) for r in range(4)]


def decrypt_block(key, block):
    """AES-128^-1 of one 16-byte block, the straightforward inverse cipher (FIPS-197 figure 12)"""
    rk = expand_key(key)
    s = [a ^ b for a, b in zip(block, rk[10])]
    for rnd in range(9, -1, -1):
        s = [s[i] for i in _INV_SHIFT]
        s = [INV_SBOX[b] for b in s]
        s = [a ^ b for a, b in zip(s, rk[rnd])]
        if rnd > 0:
            m = []
            for c in range(4):
                a = s[4 * c: 4 * c + 4]
                m += [_gmul(a[r], 14) ^ _gmul(a[(r + 1) % 4], 11) ^ _gmul(a[(r + 2) % 4], 13) ^ _gmul(a[(r + 3) % 4], 9) for r in range(4)]
            s = m
    return bytes(s)


def decrypt_blocks(key, blocks):
    """AES-128^-1 of many blocks at once: blocks uint8 [n, 16] -> uint8 [n, 16]"""
    rk = [np.frombuffer(k, dtype=np.uint8) for k in expand_key(key)]
    s = np.asarray(blocks, dtype=np.uint8).reshape(-1, 16) ^ rk[10]
    for rnd in range(9, -1, -1):
        s = _INV_NP[s[:, _INV_SHIFT]] ^ rk[rnd]
        if rnd > 0:
            a = s.reshape(-1, 4, 4)                                     # [block, column, row]
            a1, a2, a3 = np.roll(a, -1, axis=2), np.roll(a, -2, axis=2), np.roll(a, -3, axis=2)
            s = (_MUL[14][a] ^ _MUL[11][a1] ^ _MUL[13][a2] ^ _MUL[9][a3]).reshape(-1, 16)
    return s


def cbc(key, iv, data, decrypt=False):
    """AES-128-CBC of whole blocks, no padding"""
    prev, out = bytes(iv), b""
    for i in range(0, len(data), 16):
        b = bytes(data[i:i + 16])
        if decrypt:
            out += bytes(x ^ y for x, y in zip(decrypt_block(key, b), prev))
            prev = b
        else:
            prev = encrypt_block(key, bytes(x ^ y for x, y in zip(b, prev)))
            out += prev
    return out


# ---- the pattern -------------------------------------------------------------------------------------------------------------------

def pattern(c, k):
    """crypt_byte_block, skip_byte_block as the rule reads them: 0, 0 is every block"""
    return (1, 0) if c == 0 and k == 0 else (c, k)


def is_crypt(c, k, whole, nb, i):
    """block i of nb whole blocks is a crypt block (the predicate of the header's RULE)"""
    c, k = pattern(c, k)
    r = i % (c + k)
    return i < nb and r < c and (not whole or i - r + c <= nb)


def crypt_block_list(c, k, whole, nb):
    return [i for i in range(nb) if is_crypt(c, k, whole, nb, i)]


def crypt_blocks(c, k, whole, nb):
    """the closed form"""
    c, k = pattern(c, k)
    f, m = divmod(nb, c + k)
    return f * c + ((c if m >= c else 0) if whole else min(m, c))


def block_of(c, k, j):
    c, k = pattern(c, k)
    return j // c * (c + k) + j % c


def params_ok(iv_mode, flags, c, k, reserved0=0, reserved1=0):
    return iv_mode <= 1 and not flags & ~3 and c <= 15 and k <= 15 and not (c == 0 and k != 0) and reserved0 == 0 and reserved1 == 0


def sample_iv(s, iv=None, iv0=None):
    return bytes(bytearray(iv[16 * s: 16 * s + 16])) if iv0 is None else bytes(iv0)


# ---- hbs_cbcs_crypt ----------------------------------------------------------------------------------------------------------------

def crypt(data, off, size, sub_first, sub, key, iv=None, iv0=None, c=1, k=9, whole=False, decrypt=False):
    """hbs_cbcs_crypt on a copy of data (uint8 array) -> (the data behind the call, 16 x the crypt blocks)"""
    out = np.array(data, dtype=np.uint8, copy=True)
    done = 0
    for s in range(len(off)):
        p = int(off[s])
        e = sub[int(sub_first[s]): int(sub_first[s + 1])]
        for clear, protect in zip(e["clear"].tolist(), e["protect"].tolist()):
            p += clear
            blocks = crypt_block_list(c, k, whole, protect // 16)
            if blocks:
                chain = b"".join(bytes(out[p + 16 * i: p + 16 * i + 16]) for i in blocks)
                chain = np.frombuffer(cbc(key, sample_iv(s, iv, iv0), chain, decrypt), dtype=np.uint8)
                for j, i in enumerate(blocks):
                    out[p + 16 * i: p + 16 * i + 16] = chain[16 * j: 16 * j + 16]
                done += 16 * len(blocks)
            p += protect
    return out, done


def crypt_many(data, off, size, sub_first, sub, key, iv=None, iv0=None, c=1, k=9, whole=False, decrypt=False):
    """`crypt`, all entries at once"""
    out = np.array(data, dtype=np.uint8, copy=True)
    c, k = pattern(c, k)
    first = np.asarray(sub_first, dtype=np.int64)
    n_ent = int(first[-1]) if len(off) else 0
    if not n_ent:
        return out, 0
    clear, protect = sub["clear"][:n_ent].astype(np.int64), sub["protect"][:n_ent].astype(np.int64)
    sample = np.searchsorted(first, np.arange(n_ent), side="right") - 1               # the last s with first[s] <= e
    sample = np.minimum(sample, len(off) - 1)
    ends = np.cumsum(clear + protect)                                                 # over all entries; per sample: less those in front
    at_first = np.concatenate([[0], ends])[first[:-1]]
    p = np.asarray(off, dtype=np.int64)[sample] + (ends - protect) - at_first[sample]
    nb = protect // 16
    f, m = nb // (c + k), nb % (c + k)
    n = f * c + (np.where(m >= c, c, 0) if whole else np.minimum(m, c))
    ent = np.repeat(np.arange(n_ent), n)                                              # a row per crypt block: its entry, its number
    if not len(ent):
        return out, 0
    j = np.arange(len(ent)) - np.repeat(np.cumsum(n) - n, n)
    addr = p[ent] + 16 * (j // c * (c + k) + j % c)
    idx = addr[:, None] + np.arange(16)
    blocks = out[idx]
    ivs = np.frombuffer(bytes(iv0), dtype=np.uint8)[None, :].repeat(len(off), 0) if iv0 is not None else np.asarray(iv, dtype=np.uint8).reshape(-1, 16)
    head = j == 0
    if decrypt:
        prev = np.empty_like(blocks)
        prev[1:] = blocks[:-1]
        prev[head] = ivs[sample[ent[head]]]
        out[idx] = decrypt_blocks(key, blocks) ^ prev
    else:
        order = np.argsort(j, kind="stable")                                          # the rows by number: step j is a slice
        cuts = np.searchsorted(j[order], np.arange(int(j.max()) + 2))
        rows = order[cuts[0]:cuts[1]]
        prev_rows, prev = rows, encrypt_blocks(key, blocks[rows] ^ ivs[sample[ent[rows]]])
        out[idx[rows]] = prev
        for step in range(1, int(j.max()) + 1):
            rows = order[cuts[step]:cuts[step + 1]]                                   # the chains that go on: rows - 1 are among prev_rows
            keep = np.searchsorted(prev_rows, rows - 1)
            prev = encrypt_blocks(key, blocks[rows] ^ prev[keep])
            out[idx[rows]] = prev
            prev_rows = rows
    return out, 16 * int(n.sum())
