#!/usr/bin/env python3
"""Golden fixture for the steered X25519 cases of tests/x25519_steer.py, generated in the build
container with libsodium 1.0.18 (the library make_golden_x25519.py uses): an implementation
independent of the big-integer reference, of the oracle and of the device code.

Cases: every steered target of x25519_steer.steered_cases under its three scalars (the outputs are
small or all-ones numbers, on which a hand-written final reduction takes its rare branches), the
non-canonical u = p + 18 and 2^255 - 1 with and without bit 255, and the extreme scalars on the
base point.  libsodium's crypto_scalarmult returns -1 for the all-zero outputs of low-order
points; those stay with the big-integer reference and are not in the file.
Writes tests/golden/x25519_edges.json.
"""
import ctypes
import glob
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import x25519_steer as xs  # noqa: E402

S = ctypes.CDLL(sorted(glob.glob("/opt/conda/lib/libsodium.so*"))[0])
assert S.sodium_init() >= 0


def x25519(k, u):
    out = ctypes.create_string_buffer(32)
    assert S.crypto_scalarmult(out, k, u) == 0
    return out.raw


def b(v):
    return v.to_bytes(32, "little")


def main():
    cases = []
    for k in xs.SCALARS:
        for name, t, u in xs.steered_cases(k):
            out = x25519(k, u)
            assert out == b(t), (name, t)
            cases.append({"class": name, "k": k.hex(), "u": u.hex(), "out": out.hex()})
        for v in (xs.P + 18, (1 << 255) - 1):
            for hi in (0, 1 << 255):
                cases.append({"class": "non-canonical u", "k": k.hex(), "u": b(v | hi).hex(),
                              "out": x25519(k, b(v | hi)).hex()})
    nine = b(9)
    for name, k in (("zero", bytes(32)), ("ones", b"\xff" * 32), ("bits 0..2", b(7)), ("bit 255", b(1 << 255)),
                    ("alternating", b"\x55" * 32), ("runs", (b"\xff" * 4 + bytes(4)) * 4)):
        cases.append({"class": "scalar " + name, "k": k.hex(), "u": nine.hex(), "out": x25519(k, nine).hex()})
    out = {"generator": "libsodium 1.0.18 via tests/golden/make_golden_x25519_edges.py", "cases": cases}
    with open(os.path.join(HERE, "x25519_edges.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("x25519 edges %d" % len(cases))


if __name__ == "__main__":
    main()
