"""Writes tests/golden/cbcs/vectors.json once: random plaintexts of a few hundred bytes as one protected range each, with their
ciphertext at 1:9, 1:0 and 3:7, with and without HBS_CBCS_WHOLE_RUNS.  The cipher is the local openssl's (enc -aes-128-cbc
-nopad over the crypt blocks of the range, which the pattern rule of tests/_cbcs_ref.py picks), so the recorded bytes do not come
from the reference's own AES; tests/test_cbcs_ref.py reads them on machines without openssl.

    python -m tests.tools.make_cbcs_golden
"""
import json
import os
import shutil
import subprocess

import numpy as np

from tests import _cbcs_ref as R

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "cbcs", "vectors.json")


def openssl_cbc(exe, key, iv, data):
    run = subprocess.run([exe, "enc", "-aes-128-cbc", "-nopad", "-K", key.hex(), "-iv", iv.hex()], input=data, capture_output=True, check=True)
    return run.stdout


def main():
    exe = shutil.which("openssl")
    if not exe:
        raise SystemExit("no openssl binary")
    rng = np.random.default_rng(2401)
    rows = []
    for length in (16, 47, 160, 175, 208, 333, 480, 641):
        key, iv = (bytes(rng.integers(0, 256, 16, dtype=np.uint8)) for _ in range(2))
        plain = bytes(rng.integers(0, 256, length, dtype=np.uint8))
        for c, k in ((1, 9), (1, 0), (3, 7)):
            for whole in (0, 1):
                blocks = R.crypt_block_list(c, k, whole, length // 16)
                out = bytearray(plain)
                if blocks:
                    enc = openssl_cbc(exe, key, iv, b"".join(plain[16 * i: 16 * i + 16] for i in blocks))
                    for j, i in enumerate(blocks):
                        out[16 * i: 16 * i + 16] = enc[16 * j: 16 * j + 16]
                rows.append(dict(key=key.hex(), iv=iv.hex(), crypt_byte_block=c, skip_byte_block=k, whole_runs=whole, plain=plain.hex(),
                                 cipher=bytes(out).hex()))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(rows, f, indent=0)
        f.write("\n")
    print("%d vectors -> %s" % (len(rows), OUT))


if __name__ == "__main__":
    main()
