"""tests/_cenc_ref.py against published vectors (FIPS-197 C.1, SP 800-38A F.5.1), the no-carry rule of the `cenc` counter, the
local openssl where there is one, and the subsample rule of hbs_cenc_subsamples on hand-written cases."""
import shutil
import subprocess

import numpy as np
import pytest

from tests import _cenc_ref as R

H = bytes.fromhex
KEY_38A = H("2b7e151628aed2a6abf7158809cf4f3c")
PLAIN_38A = H("6bc1bee22e409f96e93d7e117393172a" "ae2d8a571e03ac9c9eb76fac45af8e51"
              "30c81c46a35ce411e5fbc1191a0a52ef" "f69f2445df4f9b17ad2b417be66c3710")
CIPHER_38A = H("874d6191b620e3261bef6864990db6ce" "9806f66b7970fdff8617187bb9fffdff"
               "5ae4df3edbd5d35e5b4f09020db03eab" "1e031dda2fbe03d1792170a0f3009cee")
CTR_38A = H("f0f1f2f3f4f5f6f7f8f9fafbfcfdfeff")
CTR_WRAP = H("00000000000000" "01" + "ff" * 8)
WRAP_OUT = H("9e582c699ddc0085c0d36b60e14c06d0" "dc0a3bc38609c26f6f2a63a39cf7ee93")


def test_sbox_is_the_published_one():
    assert R.SBOX[:8] == [0x63, 0x7C, 0x77, 0x7B, 0xF2, 0x6B, 0x6F, 0xC5] and R.SBOX[0xFF] == 0x16 and R.SBOX[0x53] == 0xED
    assert sorted(R.SBOX) == list(range(256))


def test_fips_197_c1():
    key, block = bytes(range(16)), H("00112233445566778899aabbccddeeff")
    assert R.encrypt_block(key, block).hex() == "69c4e0d86a7b0430d8cdb78070b4c55a"
    assert bytes(R.encrypt_blocks(key, np.frombuffer(block, dtype=np.uint8))[0]).hex() == "69c4e0d86a7b0430d8cdb78070b4c55a"
    assert R.expand_key(H("2b7e151628aed2a6abf7158809cf4f3c"))[10].hex() == "d014f9a8c9ee2589e13f0cc8b6630ca6"      # FIPS-197 A.1, w40..w43


def test_sp800_38a_f51():
    ks = R.keystream(KEY_38A, CTR_38A, 64)
    assert bytes(ks ^ np.frombuffer(PLAIN_38A, dtype=np.uint8)) == CIPHER_38A


def test_counter_wraps_without_a_carry():
    assert bytes(R.keystream(KEY_38A, CTR_WRAP, 32)) == WRAP_OUT
    assert R.encrypt_block(KEY_38A, H("00000000000000" "01" + "00" * 8)) == WRAP_OUT[16:]
    assert R.encrypt_block(KEY_38A, H("00000000000000" "02" + "00" * 8)).hex() == "d4ccbed38df03f156b7a8a31966d9c0f"
    assert bytes(R.counter_blocks(CTR_WRAP, 2)[1]) == H("00000000000000" "01" + "00" * 8)


def test_many_blocks_agree_with_one_at_a_time():
    rng = np.random.default_rng(23)
    key = bytes(rng.integers(0, 256, 16, dtype=np.uint8))
    blocks = rng.integers(0, 256, (40, 16), dtype=np.uint8)
    many = R.encrypt_blocks(key, blocks)
    for b, m in zip(blocks, many):
        assert R.encrypt_block(key, bytes(b)) == bytes(m)


def test_sequential_ivs():
    iv0 = H("ff" * 7 + "fe") + H("aa" * 8)
    assert [R.sample_ctr(s, iv0=iv0).hex() for s in range(3)] == ["ff" * 7 + "fe" + "00" * 8, "ff" * 8 + "00" * 8, "00" * 16]


def test_against_openssl(tmp_path):
    exe = shutil.which("openssl")
    if not exe:
        pytest.skip("no openssl binary")
    rng = np.random.default_rng(7)
    key = bytes(rng.integers(0, 256, 16, dtype=np.uint8))
    blocks = rng.integers(0, 256, (300, 16), dtype=np.uint8)
    src = tmp_path / "blocks.bin"
    src.write_bytes(blocks.tobytes())
    run = subprocess.run([exe, "enc", "-aes-128-ecb", "-nopad", "-K", key.hex(), "-in", str(src)], capture_output=True, timeout=60)
    if run.returncode != 0:
        pytest.skip("openssl has no aes-128-ecb: " + run.stderr.decode(errors="replace")[-200:])
    assert run.stdout == R.encrypt_blocks(key, blocks).tobytes()


# ---- the subsample rule, by hand ---------------------------------------------------------------------------------------------------

SEI, SLICE = 39, 1


def test_clear_count_splits_at_65535():
    L = 4
    # an SEI in front of a slice of 100 bytes with a clear lead of 10: C = SEI record + L + 10, P = 90
    for sei, want in ((65535 - 4 - 14, [(65535, 90)]), (65536 - 4 - 14, [(65535, 0), (1, 90)]), (131070 - 4 - 14, [(65535, 0), (65535, 90)]),
                      (131071 - 4 - 14, [(65535, 0), (65535, 0), (1, 90)])):
        assert R.sample_subsamples([(sei, SEI, None), (100, SLICE, 10)], L) == want
    # ... and as a trailing run
    assert R.sample_subsamples([(65535 - 4, SEI, None)], L) == [(65535, 0)]
    assert R.sample_subsamples([(65536 - 4, SEI, None)], L) == [(65535, 0), (1, 0)]
    assert R.sample_subsamples([(131070 - 4, SEI, None)], L) == [(65535, 0), (65535, 0)]


def test_zero_clear_trailing_and_empty():
    assert R.emit([], 0, 5) is None
    out = []
    R.emit(out, 0, 5)
    assert out == [(0, 5)]
    assert R.sample_subsamples([], 4) == []
    assert R.sample_subsamples([(0, 63, None)], 1) == [(1, 0)]                               # an empty NAL is its length field
    assert R.sample_subsamples([(50, SLICE, 8), (20, SEI, None)], 2) == [(10, 42), (22, 0)]    # the trailing (C, 0)
    assert R.sample_subsamples([(50, SLICE, None), (60, SLICE, None)], 4, clear_lead=2) == [(6, 48), (6, 58)]
    assert R.sample_subsamples([(50, SLICE, None)], 4, clear_lead=96) == [(54, 0)]            # the lead is the whole NAL


def test_align16():
    assert R.sample_subsamples([(50, SLICE, 8)], 4, flags=R.ALIGN16) == [(4 + 8 + 10, 32)]
    assert R.sample_subsamples([(23, SLICE, 8), (40, SLICE, 8)], 4, flags=R.ALIGN16) == [(4 + 23 + 4 + 8, 32)]      # P = 15 < 16: wholly clear
    assert R.sample_subsamples([(23, SLICE, 8)], 4, flags=R.ALIGN16) == [(27, 0)]
    assert R.sample_subsamples([(24, SLICE, 8)], 4, flags=R.ALIGN16) == [(12, 16)]


def test_table_over_access_units():
    # NALs: AU 0 = SEI + slice, AU 1 = nothing kept, AU 2 = slice; type byte = type << 1
    stream = np.zeros(100, dtype=np.uint8)
    starts, ends = np.array([4, 20, 50, 70]), np.array([16, 46, 60, 100])
    stream[4], stream[20], stream[50], stream[70] = SEI << 1, SLICE << 1, 35 << 1, 19 << 1
    nal_au = np.array([7, 7, 8, 9], dtype=np.uint32)
    keep = np.array([1, 1, 0, 1], dtype=np.uint8)
    po = np.array([R.M64, 25, R.M64, 72], dtype=np.uint64)
    r = R.subsamples(stream, starts, ends, nal_au, 3, 4, keep=keep, payload_off=po)
    assert r["error"] == 0 and r["sub_first"].tolist() == [0, 1, 1, 2]
    assert r["sub"].tolist() == [(16 + 4 + 5, 21), (4 + 2, 28)]
    assert (r["protected"], r["sample_bytes"], r["kept"]) == (49, 16 + 30 + 34, 3)
    assert R.subsamples(stream, starts, ends, nal_au, 3, 4, keep=keep, payload_off=po, sub_cap=1)["error"] == R.E_CAPACITY
    for value in (R.M64, 71, 101):
        po2 = po.copy()
        po2[3] = value
        assert R.subsamples(stream, starts, ends, nal_au, 3, 4, keep=keep, payload_off=po2)["bad"] == 4
    assert R.subsamples(stream, starts, ends, nal_au, 4, 4)["bad"] == 4                      # the last AU number


def test_crypt_is_its_own_inverse_and_leaves_clear_bytes():
    rng = np.random.default_rng(5)
    data = rng.integers(0, 256, 200, dtype=np.uint8)
    off, size = np.array([3, 120], dtype=np.uint64), np.array([100, 40], dtype=np.uint64)
    sub = np.array([(5, 7), (3, 30), (0, 1), (54, 0), (10, 30)], dtype=R.SUBSAMPLE)
    first = np.array([0, 4, 5], dtype=np.uint64)
    assert R.crypt_check(200, off, size, first, sub) == 0
    key = bytes(range(16))
    out, done, used = R.crypt(data, off, size, first, sub, key, iv0=bytes(8))
    assert done == 68 and bytes(used[1]) == bytes(7) + b"\x01" + bytes(8)
    mask = np.zeros(200, dtype=bool)
    for a, b in ((8, 15), (18, 48), (48, 49), (130, 160)):
        mask[a:b] = True
    assert (out[~mask] == data[~mask]).all() and (out[mask] != data[mask]).any()
    ks = R.keystream(key, bytes(16), 38)
    assert (out[18:48] == data[18:48] ^ ks[7:37]).all() and out[48] == data[48] ^ ks[37]     # the keystream runs on across entries
    back, _, _ = R.crypt(out, off, size, first, sub, key, iv0=bytes(8))
    assert (back == data).all()
    assert R.crypt_check(200, off, np.array([101, 40], dtype=np.uint64), first, sub) == 1
    assert R.crypt_check(150, off, size, first, sub) == 2
