"""tests/_cbcs_ref.py against published vectors (FIPS-197 C.1 in both directions, SP 800-38A F.2.1 / F.2.2), its batched form
against its sequential one, the local openssl where there is one, the recorded vectors of tests/golden/cbcs (written once by
tests/tools/make_cbcs_golden.py with openssl's cipher), and the pattern predicate against the closed form."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import _cbcs_ref as R

H = bytes.fromhex
KEY_38A = H("2b7e151628aed2a6abf7158809cf4f3c")
IV_38A = bytes(range(16))
PLAIN_38A = H("6bc1bee22e409f96e93d7e117393172a" "ae2d8a571e03ac9c9eb76fac45af8e51"
              "30c81c46a35ce411e5fbc1191a0a52ef" "f69f2445df4f9b17ad2b417be66c3710")
CBC_38A = H("7649abac8119b246cee98e9b12e9197d" "5086cb9b507219ee95db113a917678b2"
            "73bed6b8e3c1743b7116e69e22229516" "3ff1caa1681fac09120eca307586e1a7")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cbcs", "vectors.json")


def one_entry(nbytes, lead=0):
    return (np.array([lead], dtype=np.uint64), np.array([nbytes], dtype=np.uint64), np.array([0, 1], dtype=np.uint64),
            np.array([(0, nbytes)], dtype=R.SUBSAMPLE))


def test_inverse_sbox():
    assert sorted(R.INV_SBOX) == list(range(256)) and R.INV_SBOX[0x63] == 0 and R.INV_SBOX[0] == 0x52 and R.INV_SBOX[0xED] == 0x53
    assert all(R.INV_SBOX[R.SBOX[x]] == x for x in range(256))


def test_fips_197_c1_both_directions():
    key, plain, cipher = bytes(range(16)), H("00112233445566778899aabbccddeeff"), H("69c4e0d86a7b0430d8cdb78070b4c55a")
    assert R.encrypt_block(key, plain) == cipher and R.decrypt_block(key, cipher) == plain
    assert bytes(R.decrypt_blocks(key, np.frombuffer(cipher, dtype=np.uint8))[0]) == plain


def test_sp800_38a_f21_f22():
    assert R.cbc(KEY_38A, IV_38A, PLAIN_38A) == CBC_38A
    assert R.cbc(KEY_38A, IV_38A, CBC_38A, decrypt=True) == PLAIN_38A
    # as one entry at 1:0, in front of a tail that stays clear
    data = np.frombuffer(b"\xC3" * 5 + PLAIN_38A + b"tail!", dtype=np.uint8)
    off, size, first, sub = one_entry(69, lead=5)
    for fn in (R.crypt, R.crypt_many):
        enc, done = fn(data, off, size, first, sub, KEY_38A, iv0=IV_38A, c=1, k=0)
        assert done == 64 and bytes(enc) == b"\xC3" * 5 + CBC_38A + b"tail!"
        dec, done = fn(enc, off, size, first, sub, KEY_38A, iv=np.frombuffer(IV_38A, dtype=np.uint8), c=0, k=0, decrypt=True)
        assert done == 64 and bytes(dec) == bytes(data)
    # 1:9 over the same bytes: the first block alone
    enc, done = R.crypt(data, off, size, first, sub, KEY_38A, iv0=IV_38A)
    assert done == 16 and bytes(enc) == b"\xC3" * 5 + CBC_38A[:16] + PLAIN_38A[16:] + b"tail!"


def test_many_blocks_agree_with_one_at_a_time():
    rng = np.random.default_rng(29)
    key = bytes(rng.integers(0, 256, 16, dtype=np.uint8))
    blocks = rng.integers(0, 256, (40, 16), dtype=np.uint8)
    many = R.decrypt_blocks(key, blocks)
    for b, m in zip(blocks, many):
        assert R.decrypt_block(key, bytes(b)) == bytes(m)
    assert np.array_equal(R.decrypt_blocks(key, R.encrypt_blocks(key, blocks)), blocks)


def random_case(rng, n_samples=12):
    subs, first, off, size, at = [], [0], [], [], int(rng.integers(0, 40))
    for _ in range(n_samples):
        e = [(int(rng.integers(0, 50)) if rng.integers(0, 3) else 0, int(rng.integers(0, 500)) if rng.integers(0, 4) else 0)
             for _ in range(int(rng.integers(0, 5)))]
        subs += e
        first.append(len(subs))
        off.append(at)
        size.append(sum(a + b for a, b in e))
        at += size[-1] + int(rng.integers(0, 30))
    return (rng.integers(0, 256, at + 5, dtype=np.uint8), np.array(off, dtype=np.uint64), np.array(size, dtype=np.uint64),
            np.array(first, dtype=np.uint64), np.array(subs, dtype=R.SUBSAMPLE).reshape(-1))


@pytest.mark.parametrize("c,k", ((1, 9), (1, 0), (0, 0), (3, 7), (2, 1), (15, 15)))
@pytest.mark.parametrize("whole", (False, True))
def test_batched_against_sequential(c, k, whole):
    rng = np.random.default_rng(1000 + 16 * c + k)
    data, off, size, first, sub = random_case(rng)
    assert R.crypt_check(len(data), off, size, first, sub) == 0
    key = bytes(rng.integers(0, 256, 16, dtype=np.uint8))
    iv = rng.integers(0, 256, 16 * len(off), dtype=np.uint8)
    for kw in (dict(iv=iv), dict(iv0=bytes(iv[:16]))):
        enc, done = R.crypt(data, off, size, first, sub, key, c=c, k=k, whole=whole, **kw)
        enc2, done2 = R.crypt_many(data, off, size, first, sub, key, c=c, k=k, whole=whole, **kw)
        assert done == done2 == 16 * sum(R.crypt_blocks(c, k, whole, int(p) // 16) for p in sub["protect"]) and np.array_equal(enc, enc2)
        assert (done > 0) == (not np.array_equal(enc, data))
        for fn in (R.crypt, R.crypt_many):
            dec, done3 = fn(enc, off, size, first, sub, key, c=c, k=k, whole=whole, decrypt=True, **kw)
            assert done3 == done and np.array_equal(dec, data)


def test_chain_and_pattern_restart_at_every_entry():
    rng = np.random.default_rng(3)
    body = rng.integers(0, 256, 200, dtype=np.uint8)
    data = np.concatenate([body, body])
    off, size = np.array([0], dtype=np.uint64), np.array([400], dtype=np.uint64)
    sub = np.array([(8, 192), (8, 192)], dtype=R.SUBSAMPLE)
    enc, done = R.crypt(data, off, size, np.array([0, 2], dtype=np.uint64), sub, bytes(16), iv0=bytes(range(16)), c=1, k=9)
    assert done == 64 and np.array_equal(enc[:200], enc[200:]) and not np.array_equal(enc[:200], body)
    changed = np.flatnonzero(enc[:200] != body)
    assert changed.min() >= 8 and set(changed.tolist()) <= set(range(8, 24)) | set(range(168, 184))


def test_against_openssl(tmp_path):
    exe = shutil.which("openssl")
    if not exe:
        pytest.skip("no openssl binary")
    rng = np.random.default_rng(11)
    key, iv = (bytes(rng.integers(0, 256, 16, dtype=np.uint8)) for _ in range(2))
    plain = rng.integers(0, 256, 16 * 300, dtype=np.uint8)
    run = subprocess.run([exe, "enc", "-aes-128-cbc", "-nopad", "-K", key.hex(), "-iv", iv.hex()], input=plain.tobytes(), capture_output=True, timeout=60)
    if run.returncode != 0:
        pytest.skip("openssl has no aes-128-cbc: " + run.stderr.decode(errors="replace")[-200:])
    off, size, first, sub = one_entry(len(plain))
    enc, done = R.crypt_many(plain, off, size, first, sub, key, iv0=iv, c=1, k=0)
    assert done == len(plain) and enc.tobytes() == run.stdout
    assert R.cbc(key, iv, run.stdout[:160], decrypt=True) == plain[:160].tobytes()
    dec, _ = R.crypt_many(enc, off, size, first, sub, key, iv0=iv, c=1, k=0, decrypt=True)
    assert np.array_equal(dec, plain)


def test_recorded_vectors():
    rows = json.load(open(GOLDEN))
    assert len(rows) == 48 and {(r["crypt_byte_block"], r["skip_byte_block"], r["whole_runs"]) for r in rows} == {
        (c, k, w) for c, k in ((1, 9), (1, 0), (3, 7)) for w in (0, 1)}
    differ = 0
    for r in rows:
        plain = np.frombuffer(H(r["plain"]), dtype=np.uint8)
        off, size, first, sub = one_entry(len(plain))
        kw = dict(iv0=H(r["iv"]), c=r["crypt_byte_block"], k=r["skip_byte_block"], whole=bool(r["whole_runs"]))
        for fn in (R.crypt, R.crypt_many):
            enc, _ = fn(plain, off, size, first, sub, H(r["key"]), **kw)
            assert enc.tobytes().hex() == r["cipher"]
            dec, _ = fn(enc, off, size, first, sub, H(r["key"]), decrypt=True, **kw)
            assert np.array_equal(dec, plain)
    # the two readings of a truncated last run differ for 3:7 alone
    by = {(r["plain"], r["crypt_byte_block"], r["skip_byte_block"], r["whole_runs"]): r["cipher"] for r in rows}
    for (plain, c, k, w), cipher in by.items():
        if w == 0 and by[(plain, c, k, 1)] != cipher:
            assert (c, k) == (3, 7)
            differ += 1
    assert differ >= 2


def test_pattern_predicate_against_the_closed_form():
    for c in range(16):
        for k in range(16):
            if c == 0 and k != 0:
                assert not R.params_ok(0, 0, c, k)
                continue
            assert R.params_ok(1, 3, c, k)
            for whole in (False, True):
                for nb in range(71):
                    blocks = R.crypt_block_list(c, k, whole, nb)
                    assert len(blocks) == R.crypt_blocks(c, k, whole, nb)
                    assert blocks == [R.block_of(c, k, j) for j in range(len(blocks))]
                    if c <= 1:
                        assert blocks == R.crypt_block_list(c, k, not whole, nb)
    assert R.crypt_block_list(1, 9, False, 21) == [0, 10, 20] and R.crypt_block_list(3, 7, False, 12) == [0, 1, 2, 10, 11]
    assert R.crypt_block_list(3, 7, True, 12) == [0, 1, 2] and R.crypt_block_list(0, 0, True, 3) == [0, 1, 2]
    assert not R.params_ok(2, 0, 1, 9) and not R.params_ok(0, 4, 1, 9) and not R.params_ok(0, 0, 16, 0) and not R.params_ok(0, 0, 1, 16)
    assert not R.params_ok(0, 0, 1, 9, reserved0=1) and not R.params_ok(0, 0, 1, 9, reserved1=1)
