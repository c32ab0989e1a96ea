"""Steered X25519 inputs: points u whose shared secret X25519(k, u) is a chosen number t.

X25519 is invertible on a prime-order subgroup: when the point with x-coordinate t lies in the
subgroup of order L of the curve (cofactor 8) or of order L' of its twist (cofactor 4), then
u = x((k^-1 mod order) * Q_t) gives X25519(k, u) = t for the clamped scalar k.  About 3 in 16
targets qualify.  "The output is a small number" steers the kernel's final reduction: fe_carry
after the last fe_mul leaves p + t, not t, whenever t < 19 * (V >> 255) for the uncarried product
V, which puts the conditional subtraction of p, values >= 2^255 and the wrap of 19 into limb 0
(random inputs: probability ~2^-250) under the compiled kernel.

x25519_ref is the big-integer RFC 7748 ladder, the reference of everything here.  device_x25519
restates jeromq_amd/csrc/cz_x25519.hip line by line on Python integers, asserts every
instruction's width on the way (u32 limbs, u64 columns, no negative fe_sub limb) and reports the
branches the final reduction took, so a test can tell that its inputs reached them.  Helper module
of test_x25519_steer.py and test_gpu_x25519_edges.py; no GPU.
"""
import functools
import json
import os
import random
from operator import itemgetter, mul

P = (1 << 255) - 19
A = 486662
A24 = 121665
L_CURVE = (1 << 252) + 27742317777372353535851937790883648493
L_TWIST = (1 << 253) - 55484635554744707071703875581767296995
ORDER8 = (325606250916557431795983626356110631294008115727848805560023387167927233504,
          39382357235489614581723060781553021112529911719440698176882885853963445705823)
# a target is reachable with probability 3/16 (1/8 of the curve's x, 1/4 of the twist's): the
# chance that three reachable ones take more than 160 skips is (13/16)^160 * ~2000 < 1e-10
MAX_SKIP = 160


# ---- the reference ---------------------------------------------------------------------------
def clamp(k_bytes):
    k = int.from_bytes(k_bytes, "little")
    return (k & ~7 & ((1 << 255) - 1)) | 1 << 254


def ladder(k, u):
    """RFC 7748 section 5 Montgomery ladder over bits 254..0 of k, no clamping: (x, z) of k * (u : 1)"""
    x1, x2, z2, x3, z3, swap = u % P, 1, 0, u % P, 1, 0
    for t in range(254, -1, -1):
        kt = k >> t & 1
        if swap ^ kt:
            x2, x3, z2, z3 = x3, x2, z3, z2
        swap = kt
        a, b, c, d = x2 + z2, x2 - z2, x3 + z3, x3 - z3
        aa, bb, da, cb = a * a % P, b * b % P, d * a % P, c * b % P
        e = aa - bb
        x3 = (da + cb) ** 2 % P
        z3 = x1 * (da - cb) ** 2 % P
        x2 = aa * bb % P
        z2 = e * (aa + A24 * e) % P
    if swap:
        x2, z2 = x3, z3
    return x2, z2


def x25519_ref(k_bytes, u_bytes):
    """X25519(k, u), RFC 7748: the scalar clamped, bit 255 of u masked, a non-canonical u reduced"""
    u = int.from_bytes(u_bytes, "little") & ((1 << 255) - 1)
    x, z = ladder(clamp(k_bytes), u)
    return (x * pow(z, P - 2, P) % P).to_bytes(32, "little")


@functools.lru_cache(maxsize=None)
def subgroup_order(t):
    """The prime order of the subgroup the point(s) with x-coordinate t lie in (L on the curve, L'
    on the twist, told apart by the Legendre symbol of t^3 + A t^2 + t), or None when they lie in
    neither.  A property of t alone."""
    t %= P
    rhs = (t * t * t + A * t * t + t) % P
    if rhs == 0:
        return None                       # t = 0 and the other 2-torsion x
    order = L_CURVE if pow(rhs, (P - 1) // 2, P) == 1 else L_TWIST
    return order if ladder(order, t)[1] == 0 else None


def steer(k_bytes, t):
    """The 32-byte u with X25519(k, u) = t, or None when t's point is in no prime-order subgroup"""
    t %= P
    order = subgroup_order(t)
    if order is None:
        return None
    x, z = ladder(pow(clamp(k_bytes), -1, order), t)
    assert z != 0
    u = (x * pow(z, P - 2, P) % P).to_bytes(32, "little")
    assert x25519_ref(k_bytes, u) == t.to_bytes(32, "little")
    return u


def steer_many(k_bytes, candidates, want, max_skip=MAX_SKIP, accept=None):
    """[(t, u)] for the first `want` reachable targets among `candidates` (accept(t, u): a further
    condition).  Raises when more than max_skip candidates had to be skipped or the candidates run
    out: a case list never shrinks silently."""
    out, skipped = [], 0
    for t in candidates:
        u = steer(k_bytes, t)
        if u is not None and (accept is None or accept(t, u)):
            out.append((t % P, u))
            if len(out) == want:
                return out
        else:
            skipped += 1
            if skipped > max_skip:
                raise RuntimeError(f"{skipped} candidates skipped for {len(out)} of {want} targets")
    raise RuntimeError(f"candidates ran out at {len(out)} of {want} targets ({skipped} skipped)")


# ---- cz_x25519.hip restated ------------------------------------------------------------------
U32 = 1 << 32
U64 = 1 << 64
M26 = (1 << 26) - 1
M25 = (1 << 25) - 1
LW = (26, 25) * 5
MASK = (M26, M25) * 5
START = (0, 26, 51, 77, 102, 128, 153, 179, 204, 230)
P2 = tuple(2 * (M26 - 18) if i == 0 else 2 * MASK[i] for i in range(10))   # the limbs of 2p in fe_sub

# fe_mul's 100 terms by column: the index of a in f + f2 and of b in g + g19
# fe_sq's 55 terms by column: the index of a in f + d and of b in f + f19, those with `p <<= 1` apart
_mul = [([], []) for _ in range(10)]
_sq = [([], [], [], []) for _ in range(10)]
for _i in range(10):
    for _j in range(10):
        _k = _i + _j
        _oo = 1 if _i & 1 and _j & 1 else 0
        _mul[_k % 10][0].append(_i + 10 if _oo else _i)
        _mul[_k % 10][1].append(_j + 10 if _k >= 10 else _j)
        if _j >= _i:
            _sq[_k % 10][2 * _oo].append(_i + 10 if _i != _j else _i)
            _sq[_k % 10][2 * _oo + 1].append(_j + 10 if _k >= 10 else _j)
# as functions v -> (v[i] for the indices); an odd column of fe_sq has no odd * odd term
_MUL = [tuple(itemgetter(*x) for x in col) for col in _mul]
_SQ = [tuple(itemgetter(*x) if x else None for x in col) for col in _sq]


def limbs_value(f):
    return sum(x << s for x, s in zip(f, START))


def value_limbs(v):
    """v < 2^255 as ten limbs within their widths"""
    assert 0 <= v < 1 << 255
    return [v >> s & m for s, m in zip(START, MASK)]


def fe_carry(h):
    """u64 column sums -> limbs; the (u32) casts at the end must lose nothing"""
    h = list(h)
    for i in range(9):
        c = h[i] >> LW[i]
        h[i] &= MASK[i]
        h[i + 1] += c
        assert h[i + 1] < U64
    c = h[9] >> 25
    h[9] &= M25
    assert c * 19 < U64
    h[0] += c * 19
    assert h[0] < U64
    c = h[0] >> 26
    h[0] &= M26
    h[1] += c
    assert max(h) < U32
    return h


def fe_carry32(f, trace=None):
    f = list(f)
    assert 0 <= min(f) and max(f) < U32
    for i in range(9):
        c = f[i] >> LW[i]
        f[i] &= MASK[i]
        f[i + 1] += c
        assert f[i + 1] < U32
    c = f[9] >> 25
    f[9] &= M25
    assert c * 19 < U32
    f[0] += c * 19
    assert f[0] < U32
    c0 = f[0] >> 26
    f[0] &= M26
    f[1] += c0
    assert f[1] < U32
    if trace is not None:
        trace.update(c9=c, c0=c0)
    return f


def fe_add(f, g):
    h = [a + b for a, b in zip(f, g)]
    assert max(h) < U32
    return h


def fe_sub(f, g):
    h = []
    for a, b, p2 in zip(f, g, P2):
        t = a + p2
        assert t < U32 and t >= b, "fe_sub limb wraps"
        h.append(t - b)
    return fe_carry32(h)


def fe_mul(f, g):
    assert max(f) < U32 and max(g) < U32
    g19 = [19 * x for x in g]
    f2 = [2 * x if i & 1 else x for i, x in enumerate(f)]
    assert max(g19) < U32 and max(f2) < U32
    a, b = f + f2, g + g19
    h = [sum(map(mul, pa(a), pb(b))) for pa, pb in _MUL]     # every term < 2^64 as a u32 * u32
    assert max(h) < U64
    return fe_carry(h)


def fe_sq(f):
    assert max(f) < U32
    f19 = [19 * x for x in f]
    d = [2 * x for x in f]
    assert max(f19) < U32 and max(d) < U32
    a, b = f + d, f + f19
    # the terms are not negative, so a column below 2^64 bounds each shifted term as well
    h = [sum(map(mul, pa(a), pb(b))) + (sum(map(mul, qa(a), qb(b))) << 1 if qa else 0) for pa, pb, qa, qb in _SQ]
    assert max(h) < U64
    return fe_carry(h)


def fe_mul_small(f, k):
    assert k < U32 and max(f) < U32
    return fe_carry([x * k for x in f])


class Ops:
    """The field operations the ladder and the inversion are written in: the restated device
    arithmetic here, worst-case bounds in test_x25519_steer.py"""
    add, sub, mul, sq, mul_small = (staticmethod(f) for f in (fe_add, fe_sub, fe_mul, fe_sq, fe_mul_small))


def fe_sqn(f, n, F=Ops):
    for _ in range(n):
        f = F.sq(f)
    return f


def fe_invert(z, F=Ops):
    t0 = F.sq(z)
    t1 = fe_sqn(t0, 2, F)
    t1 = F.mul(z, t1)
    t0 = F.mul(t0, t1)
    t2 = F.sq(t0)
    t1 = F.mul(t1, t2)
    t2 = fe_sqn(t1, 5, F)
    t1 = F.mul(t2, t1)
    t2 = fe_sqn(t1, 10, F)
    t2 = F.mul(t2, t1)
    t3 = fe_sqn(t2, 20, F)
    t2 = F.mul(t3, t2)
    t2 = fe_sqn(t2, 10, F)
    t1 = F.mul(t2, t1)
    t2 = fe_sqn(t1, 50, F)
    t2 = F.mul(t2, t1)
    t3 = fe_sqn(t2, 100, F)
    t2 = F.mul(t3, t2)
    t2 = fe_sqn(t2, 50, F)
    t1 = F.mul(t2, t1)
    t1 = fe_sqn(t1, 5, F)
    return F.mul(t1, t0)


def ladder_step(x1, x2, z2, x3, z3, F=Ops):
    """One iteration of the kernel's ladder loop after the swaps: (x2, z2, x3, z3)"""
    a = F.add(x2, z2)
    b = F.sub(x2, z2)
    c = F.add(x3, z3)
    d = F.sub(x3, z3)
    aa = F.sq(a)
    bb = F.sq(b)
    da = F.mul(d, a)
    cb = F.mul(c, b)
    e = F.sub(aa, bb)
    a = F.add(da, cb)
    b = F.sub(da, cb)
    x3 = F.sq(a)
    b = F.sq(b)
    z3 = F.mul(x1, b)
    x2 = F.mul(aa, bb)
    c = F.mul_small(e, A24)
    c = F.add(aa, c)
    z2 = F.mul(e, c)
    return x2, z2, x3, z3


def fe_from_words(w):
    h = []
    for i in range(10):
        b = START[i]
        wi, sh = b >> 5, b & 31
        x = w[wi] >> sh
        if wi + 1 < 8:
            x |= w[wi + 1] << (32 - sh)
        assert x < U64
        h.append(x % U32 & MASK[i])
    return h


def fe_to_words(f, q_seed=19, q_mul=19):
    """(words, branches).  branches: q (p subtracted), ge_p / ge_2_255 (the value handed in),
    c9 / wrap0 (the first carry pass rippled out of limb 9 / carried the 19 on out of limb 0),
    pass2_changed (the second carry pass changed a limb), limb1_2_25 (limb 1 = 2^25 going into the
    q chain), limbs (going into the q chain).  q_seed / q_mul are the kernel's two constants 19,
    parameters so that a test can show which hand-built limbs tell them from a neighbour."""
    v = limbs_value(f)
    tr = {}
    h = fe_carry32(f, tr)
    h2 = fe_carry32(h)
    br = {"ge_p": v >= P, "ge_2_255": v >= 1 << 255, "c9": tr["c9"], "wrap0": tr["c0"],
          "pass2_changed": h2 != h, "limb1_2_25": h2[1] == 1 << 25, "limbs": tuple(h2)}
    h = h2
    assert h[0] + q_seed < U32
    q = (h[0] + q_seed) >> 26
    for i in range(1, 10):
        assert h[i] + q < U32
        q = (h[i] + q) >> LW[i]
    br["q"] = q
    h[0] += q_mul * q
    assert h[0] < U32
    for i in range(9):
        h[i + 1] += h[i] >> LW[i]
        assert h[i + 1] < U32
        h[i] &= MASK[i]
    h[9] &= M25
    w = [0] * 8
    for i in range(10):
        b = START[i]
        wi, sh = b >> 5, b & 31
        w[wi] |= (h[i] << sh) % U32
        if sh and wi + 1 < 8:
            w[wi + 1] |= (h[i] >> (32 - sh)) % U32
    return w, br


def device_ladder(k_bytes, u_bytes):
    """The kernel's x25519() up to the value it hands to fe_to_words: the limbs of x2 * z2^(p-2)"""
    k = [int.from_bytes(k_bytes[4 * i:4 * i + 4], "little") for i in range(8)]
    u = [int.from_bytes(u_bytes[4 * i:4 * i + 4], "little") for i in range(8)]
    k[0] &= ~7 & (U32 - 1)
    k[7] = (k[7] & 0x7fffffff) | 0x40000000
    x1 = fe_from_words(u)
    x2, z2, x3, z3 = [1] + [0] * 9, [0] * 10, list(x1), [1] + [0] * 9
    swap = 0
    for t in range(254, -1, -1):
        kt = k[t >> 5] >> (t & 31) & 1
        if swap ^ kt:
            x2, x3, z2, z3 = x3, x2, z3, z2
        swap = kt
        x2, z2, x3, z3 = ladder_step(x1, x2, z2, x3, z3)
    if swap:
        x2, z2 = x3, z3
    return fe_mul(x2, fe_invert(z2))


def device_x25519(k_bytes, u_bytes):
    """(X25519(k, u) as the kernel computes it, the branches its fe_to_words took)"""
    w, br = fe_to_words(device_ladder(k_bytes, u_bytes))
    return b"".join(x.to_bytes(4, "little") for x in w), br


# ---- targets ---------------------------------------------------------------------------------
SCALARS = tuple(random.Random(0x25519 + i).randbytes(32) for i in range(3))
PER_CLASS = 3


def _ones_2_9(low):
    """limbs 2..9 all ones over the 51 low bits `low`"""
    return (1 << 255) - (1 << 51) + low


def candidates(name):
    """The candidate targets of a class, in a fixed order (seeded where they are drawn), as groups:
    CLASSES wants its count of reachable targets from each group"""
    rng = random.Random("x25519 " + name)
    if name == "q=1":                 # arrives as p + t
        return [list(range(2, 19))]
    if name == ">=2^255":             # arrives as p + t = 2^255 + (t - 19)
        return [list(range(19, 64))]
    if name == "limb0-wrap":          # p + t has limb 0 = 2^26 - 19 + j: the 19 of the ripple carries on
        return [[m << 26 | j for m in range(1, 8) for j in range(19)]]
    if name == "limb1-ones":
        return [[M25 << 26 | j for j in range(19)] + [M25 << 26 | rng.randrange(19, 1 << 26) for _ in range(80)]]
    if name == "under-p":             # p - 2 - j, and p - 2^26 m - j
        return [[P - 2 - j for j in range(40)], [P - (rng.randrange(1, 1 << 10) << 26) - j for j in range(80)]]
    if name == "limbs2-9-ones":
        return [[_ones_2_9(rng.randrange(1 << 51) if i % 3 else rng.randrange(1 << 26)) for i in range(120)]]
    if name == "limb-starts":
        return [[(1 << s) - d for s in START[1:] for d in (1, 0)]]
    if name == "low-limbs-ones":      # limbs 0..i-1 all ones but for limb 0's last 19, any limbs above: h + 19
        return [[rng.randrange(1 << (255 - s)) << s | ((1 << s) - 1 - j) for j in list(range(19)) * 4]
                for s in START[1:]]   # carries out of limb i-1 and must stop there
    raise KeyError(name)


def low_ones(br):
    """how many low limbs would carry on a `+ 19`: limb 0 within 19 of its top, then all-ones limbs"""
    h, n = br["limbs"], 0
    if h[0] > M26 - 19:
        n = 1
        while n < 10 and h[n] == MASK[n]:
            n += 1
    return n


# class -> (targets wanted per scalar and group, what device_x25519's branches must say of each)
CLASSES = {
    "q=1": (PER_CLASS, lambda br: br["q"] == 1 and br["ge_p"] and not br["ge_2_255"]),
    ">=2^255": (PER_CLASS, lambda br: br["ge_2_255"] and br["c9"] == 1 and br["wrap0"] == 0 and br["q"] == 0),
    "limb0-wrap": (PER_CLASS, lambda br: br["ge_2_255"] and br["c9"] == 1 and br["wrap0"] == 1),
    "limb1-ones": (PER_CLASS, lambda br: br["limbs"][1] == M25 and br["q"] == 0),
    "under-p": (PER_CLASS, lambda br: br["q"] == 0 and not br["ge_p"] and br["limbs"][2:] == MASK[2:]),
    "limbs2-9-ones": (PER_CLASS, lambda br: br["q"] == 0 and br["limbs"][2:] == MASK[2:]),
    "limb-starts": (PER_CLASS, lambda br: br["q"] == 0),
    "low-limbs-ones": (1, lambda br: br["q"] == 0 and 1 <= low_ones(br) <= 9),
}


@functools.lru_cache(maxsize=None)
def steered_cases(k_bytes):
    """[(class, t, u)]: the first reachable targets of every group of every class under the scalar k"""
    out = []
    for name, (want, _) in CLASSES.items():
        for group in candidates(name):
            out += [(name, t, u) for t, u in steer_many(k_bytes, group, want)]
    return out


def load_edges():
    """tests/golden/x25519_edges.json: the cases above and some more as libsodium computes them"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "x25519_edges.json")) as f:
        return json.load(f)["cases"]
