"""GPU: the compiled X25519 at its final-reduction, carry, input and launch edges.

test_gpu_x25519.py feeds k_x25519 fixtures and random pairs, which take the rare branches of
fe_to_words -- the conditional subtraction of p, a value >= 2^255 rippling a carry through eight
all-ones limbs, the 19 wrapping on out of limb 0 -- with probability ~2^-250.  x25519_steer.py
solves for the point u whose shared secret is a chosen small or all-ones number, which steers the
reduction onto those branches (test_x25519_steer.py asserts, on the restated arithmetic, that each
class takes the branch it is named after).  Here the compiled kernel gets those inputs, among
random lanes in full waves and in a partial last wave, plus non-canonical and low-order u, extreme
scalars, every launch geometry around the 64-lane block, and a full oracle check of a random batch.

Every comparison is bit-exact against the big-integer x25519_steer.x25519_ref (for beforenm:
the oracle's HSalsa20 of it).  Every batch is one launch of at most a few hundred lanes, into an
output buffer with canary bytes on both sides.
"""
import functools
import random

import numpy as np
import pytest

import x25519_steer as xs
from cz_testlib import or_beforenm, or_hsalsa20, or_x25519
from x25519_steer import P

pytestmark = pytest.mark.gpu

NINE = (9).to_bytes(32, "little")
CANARY = 64


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch, torch.device("cuda:0")


def _b(v):
    return v.to_bytes(32, "little")


@functools.lru_cache(maxsize=None)
def ref(k, u):
    return xs.x25519_ref(k, u)


@functools.lru_cache(maxsize=None)
def hsalsa(shared):
    return or_hsalsa20(bytes(16), shared)


def _run(torch_dev, ks, us, beforenm=0, stream=None):
    """One launch: out[i] = X25519(ks[i], us[i]) (us None: the base point), or beforenm(pk = us[i],
    sk = ks[i]).  The output lies between two canaries, which must survive."""
    torch, dev = torch_dev
    from jeromq_amd import _lib
    n = len(ks)
    dk = torch.from_numpy(np.frombuffer(b"".join(ks), dtype=np.uint8).copy()).to(dev)
    du = None if us is None else torch.from_numpy(np.frombuffer(b"".join(us), dtype=np.uint8).copy()).to(dev)
    buf = torch.full((32 * n + 2 * CANARY,), 0xA5, dtype=torch.uint8, device=dev)
    out = buf[CANARY:CANARY + 32 * n]
    torch.cuda.synchronize()
    L = _lib.lib()
    sp = None if stream is None else stream.cuda_stream
    if beforenm:
        rc = L.cz_beforenm_batch(du.data_ptr(), dk.data_ptr(), out.data_ptr(), n, sp)
    else:
        rc = L.cz_x25519_batch(dk.data_ptr(), None if du is None else du.data_ptr(), out.data_ptr(), n, sp)
    _lib.check(rc, "x25519 batch")
    torch.cuda.synchronize()
    o = buf.cpu().numpy().tobytes()
    assert o[:CANARY] == b"\xa5" * CANARY and o[CANARY + 32 * n:] == b"\xa5" * CANARY, "canary overwritten"
    return [o[CANARY + 32 * i:CANARY + 32 * i + 32] for i in range(n)]


def _check(torch_dev, lanes, beforenm, **kw):
    """lanes: [(name, k, u)]; every lane of one launch against the reference"""
    got = _run(torch_dev, [k for _, k, _ in lanes], [u for _, _, u in lanes], beforenm, **kw)
    for (name, k, u), g in zip(lanes, got):
        want = ref(k, u)
        assert g == (hsalsa(want) if beforenm else want), (name, k.hex(), u.hex())


def _random_lanes(n, seed):
    rng = random.Random(seed)
    return [("random", rng.randbytes(32), rng.randbytes(32)) for _ in range(n)]


# ---- steered targets -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def steered_lanes():
    """Every class of x25519_steer.CLASSES under three scalars, alternating with random lanes: four
    full waves, and a partial last wave that holds every case of one scalar again"""
    edges = [(f"{name} t={t:#x}", k, u) for k in xs.SCALARS for name, t, u in xs.steered_cases(k)]
    rnd = iter(_random_lanes(320, 1))
    lanes = []
    for e in edges:
        lanes += [e, next(rnd)]
    assert len(lanes) <= 256
    while len(lanes) < 256:
        lanes.append(next(rnd))
    tail = [e for e in edges if e[1] == xs.SCALARS[-1]]
    for i, e in enumerate(tail):
        lanes.append(e)
        if i % 8 != 7:
            lanes.append(next(rnd))
    assert len(lanes) > 256 and len(lanes) % 64
    return lanes


@pytest.mark.parametrize("beforenm", (0, 1), ids=("x25519", "beforenm"))
def test_steered_targets(torch_dev, beforenm):
    lanes = steered_lanes()
    for name, k, u in lanes:                 # the targets are what the reference says
        if name != "random":
            assert int.from_bytes(ref(k, u), "little") == int(name.split("t=")[1], 16)
    _check(torch_dev, lanes, beforenm)


def test_steered_targets_single_calls(torch_dev):
    """cz_scalarmult and cz_box_beforenm (one lane, the thread's own stream): one target per class"""
    from jeromq_amd.curve import Curve, scalarmult
    k = xs.SCALARS[0]
    seen = set()
    c = Curve()
    for name, t, u in xs.steered_cases(k):
        if name in seen:
            continue
        seen.add(name)
        assert scalarmult(k, u) == _b(t), name
        out = bytearray(32)
        assert c.beforenm(out, u, k) == 0 and bytes(out) == hsalsa(_b(t)), name
    assert seen == set(xs.CLASSES)
    assert scalarmult(k, _b(xs.ORDER8[0])) == bytes(32)
    out = bytearray(32)
    assert c.beforenm(out, _b(xs.ORDER8[1]), k) == 0 and bytes(out) == hsalsa(bytes(32))


def test_libsodium_edge_fixture(torch_dev):
    edges = xs.load_edges()
    got = _run(torch_dev, [bytes.fromhex(e["k"]) for e in edges], [bytes.fromhex(e["u"]) for e in edges])
    for e, g in zip(edges, got):
        assert g.hex() == e["out"], e["class"]


# ---- non-canonical and boundary u ----------------------------------------------------------------
LOW_ORDER = (0, 1, P - 1, P, P + 1) + xs.ORDER8
BOUNDARY_U = (P - 1, P, P + 1, P + 18, (1 << 255) - 1, 0, 1) + xs.ORDER8


@pytest.mark.parametrize("beforenm", (0, 1), ids=("x25519", "beforenm"))
def test_noncanonical_and_boundary_u(torch_dev, beforenm):
    lanes = []
    for k in xs.SCALARS:
        for v in BOUNDARY_U:
            for hi in (0, 1 << 255):
                lanes.append((f"u={v:#x} bit255={hi >> 255}", k, _b(v | hi)))
                if v in LOW_ORDER:           # the reference gives 32 zero bytes; beforenm is HSalsa20 of zeros
                    assert ref(k, _b(v | hi)) == bytes(32)
                else:
                    assert ref(k, _b(v | hi)) == ref(k, _b(18))     # p + 18 and 2^255 - 1 are both 18
    _check(torch_dev, lanes, beforenm)
    got = _run(torch_dev, [xs.SCALARS[0]] * 2, [_b(P), _b(xs.ORDER8[1] | 1 << 255)], beforenm)
    assert got == [hsalsa(bytes(32)) if beforenm else bytes(32)] * 2


def test_u_bits_around_limb_and_word_starts(torch_dev):
    """fe_from_words: u = 2^i and its complement in 255 bits, for the bits on either side of every
    limb start and every 32-bit word start, and bits 254 and 255 (every bit: test_x25519_steer.py)"""
    bits = {s + d for s in xs.START[1:] for d in (-1, 0, 1)} | {32 * j + d for j in range(1, 8) for d in (-1, 0)}
    bits |= {0, 1, 253, 254, 255}
    k = xs.SCALARS[1]
    lanes = [(f"bit {i}", k, _b(u)) for i in sorted(bits) for u in (1 << i, ((1 << 255) - 1 - (1 << i)) % (1 << 256))]
    _check(torch_dev, lanes, 0)


# ---- scalar edges --------------------------------------------------------------------------------
SCALAR_EDGES = {
    "zero": bytes(32),                                   # clamps to 2^254
    "ones": b"\xff" * 32,
    "bits0-2": _b(7),                                    # all cleared by the clamp
    "bit255": _b(1 << 255),
    "bit254": _b(1 << 254),
    "alternating-55": b"\x55" * 32,
    "alternating-aa": b"\xaa" * 32,
    "run-low-half": b"\xff" * 16 + bytes(16),
    "run-high-half": bytes(16) + b"\xff" * 16,
    "runs-of-32": (b"\xff" * 4 + bytes(4)) * 4,
    "runs-of-64": (bytes(8) + b"\xff" * 8) * 2,
    "ones-but-bit-128": _b((1 << 256) - 1 - (1 << 128)),
    "one-bit-3": _b(8),
    "word-edges": _b(sum(1 << (32 * i) | 1 << (32 * i + 31) for i in range(8))),
}


def test_scalar_edges(torch_dev):
    rng = random.Random(2)
    u_rand, u_non = rng.randbytes(32), _b(P + 5 | 1 << 255)
    u_steer = xs.steered_cases(xs.SCALARS[0])[0][2]
    lanes = [(f"k={name} u={un}", k, u) for name, k in SCALAR_EDGES.items()
             for un, u in (("9", NINE), ("random", u_rand), ("non-canonical", u_non), ("a-steered-u", u_steer))]
    _check(torch_dev, lanes, 0)
    _check(torch_dev, lanes, 1)
    ks = list(SCALAR_EDGES.values())
    assert _run(torch_dev, ks, None) == [ref(k, NINE) for k in ks]     # the base point path


# ---- launch geometry -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def geometry_lanes():
    return _random_lanes(129, 3)


@pytest.mark.parametrize("count", (1, 63, 64, 65, 129))
def test_launch_geometry(torch_dev, count):
    """a different input in every lane, so a lane that reads or writes another lane's slot shows;
    the canaries of _run show a write past 32 * count"""
    lanes = geometry_lanes()[-count:]
    _check(torch_dev, lanes, 0)
    _check(torch_dev, lanes, 1)
    ks = [k for _, k, _ in lanes]
    assert _run(torch_dev, ks, None) == [ref(k, NINE) for k in ks]


def test_non_default_stream(torch_dev):
    torch, dev = torch_dev
    s = torch.cuda.Stream(device=dev)
    assert s.cuda_stream != 0
    lanes = geometry_lanes()[:65]
    _check(torch_dev, lanes, 0, stream=s)
    _check(torch_dev, lanes, 1, stream=s)


def test_empty_batch_and_null_pointers(torch_dev):
    torch, dev = torch_dev
    from jeromq_amd import _lib
    L = _lib.lib()
    assert L.cz_x25519_batch(None, None, None, 0, None) == _lib.CZ_OK
    assert L.cz_beforenm_batch(None, None, None, 0, None) == _lib.CZ_OK
    d = torch.zeros(64, dtype=torch.uint8, device=dev)
    p = d.data_ptr()
    assert L.cz_x25519_batch(None, p, p + 32, 1, None) == _lib.CZ_EINVAL       # null scalars
    assert L.cz_x25519_batch(p, None, None, 1, None) == _lib.CZ_EINVAL         # null output
    assert L.cz_beforenm_batch(None, p, p + 32, 1, None) == _lib.CZ_EINVAL     # null public keys
    assert L.cz_beforenm_batch(p, None, p + 32, 1, None) == _lib.CZ_EINVAL     # null secret keys
    assert L.cz_beforenm_batch(p, p, None, 1, None) == _lib.CZ_EINVAL
    torch.cuda.synchronize()
    assert not d.cpu().numpy().any()


# ---- a random batch, every lane ---------------------------------------------------------------------
def test_random_batch_every_lane_vs_oracle(torch_dev):
    rng = np.random.default_rng(0x25519E)
    n = 2048
    ks = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)]
    us = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)]   # incl. non-canonical u
    got = _run(torch_dev, ks, us)
    for i in range(n):
        assert got[i] == or_x25519(ks[i], us[i]), i
    got = _run(torch_dev, ks, us, beforenm=1)
    for i in range(n):
        assert got[i] == or_beforenm(us[i], ks[i]), i
