"""CPU: the X25519 reference, steering and the restated device arithmetic of x25519_steer.py.

The big-integer ladder and the line-by-line restatement of cz_x25519.hip are pinned to the
libsodium fixtures and to the oracle; steered inputs land on their targets under all three and take
the branch of the final reduction their class is named after (the conditional subtraction of p,
values >= 2^255, the wrap of 19 out of limb 0, all-ones limbs), which no fixture and no random
input reaches.  The kernel's header claims -- fe_mul / fe_sq inputs below 2^27, columns below 2^63,
fe_sub never negative -- are checked as a fixed point of interval arithmetic over the ladder step,
the inversion and the final product, and the same bounds show that the second fe_carry32 pass of
fe_to_words never changes a limb the kernel can hand it.  The compiled kernel gets the same inputs
in test_gpu_x25519_edges.py.
"""
import itertools

import pytest

import x25519_steer as xs
from cz_testlib import load_x25519_golden, or_x25519
from x25519_steer import LW, M25, M26, MASK, P, P2, U32, U64

X = load_x25519_golden()


def _b(v):
    return (v % (1 << 256)).to_bytes(32, "little")


def _words(w):
    return b"".join(x.to_bytes(4, "little") for x in w)


# ---- the reference and the restatement ---------------------------------------------------------
def test_reference_and_restatement_match_fixtures_and_oracle():
    for v in X["x25519"]:
        k, u = bytes.fromhex(v["k"]), bytes.fromhex(v["u"])
        assert xs.x25519_ref(k, u).hex() == v["out"], v["case"]
        got, br = xs.device_x25519(k, u)
        assert got.hex() == v["out"], v["case"]
        assert or_x25519(k, u).hex() == v["out"], v["case"]
        assert not br["pass2_changed"] and not br["limb1_2_25"]
        # what the steered classes below are for: no fixture subtracts p or reaches 2^255
        assert br["q"] == 0 and not br["ge_p"] and not br["ge_2_255"], v["case"]
    k = u = _b(9)
    k, u = xs.x25519_ref(k, u), k
    assert k.hex() == X["iterated_1"]


def test_steer_refuses_what_no_clamped_scalar_reaches():
    k = xs.SCALARS[0]
    for t in (0, 1, P - 1) + xs.ORDER8:                     # the low-order x-coordinates
        assert xs.steer(k, t) is None
    # p, p + 1 are 0, 1 again
    assert xs.steer(k, P) is None and xs.steer(k, P + 1) is None
    # 3 in 16: 1/8 of the curve's x-coordinates and 1/4 of the twist's
    reach = sum(xs.subgroup_order(t) is not None for t in range(1000, 1400))
    assert 400 * 3 / 16 - 4 * 8 < reach < 400 * 3 / 16 + 4 * 8      # +- 4 sigma, sigma = sqrt(400 * 3/16 * 13/16) < 8


def test_steer_many_never_shrinks_silently():
    k = xs.SCALARS[0]
    got = xs.steer_many(k, range(2, 19), 3)
    assert [t for t, _ in got] == [2, 9, 16]
    with pytest.raises(RuntimeError, match="ran out"):
        xs.steer_many(k, range(2, 19), 4)
    with pytest.raises(RuntimeError, match="skipped"):
        xs.steer_many(k, range(2, 19), 3, max_skip=5)
    with pytest.raises(RuntimeError):
        xs.steer_many(k, range(2, 19), 3, accept=lambda t, u: t != 9)


@pytest.mark.parametrize("ki", range(len(xs.SCALARS)))
def test_steered_inputs_land_on_their_targets_and_branches(ki):
    k = xs.SCALARS[ki]
    cases = xs.steered_cases(k)
    per_class = {}
    for name, t, u in cases:
        want = t.to_bytes(32, "little")
        assert xs.x25519_ref(k, u) == want, (name, t)
        assert or_x25519(k, u) == want, (name, t)
        got, br = xs.device_x25519(k, u)
        assert got == want, (name, t, br)
        assert xs.CLASSES[name][1](br), (name, hex(t), br)
        assert not br["pass2_changed"] and not br["limb1_2_25"], (name, t)
        per_class[name] = per_class.get(name, 0) + 1
    assert set(per_class) == set(xs.CLASSES) and min(per_class.values()) >= 3, per_class
    # both forms of "just under p"
    under = [t for name, t, _ in cases if name == "under-p"]
    assert sum(t >= P - 64 for t in under) >= 3 and sum(t < P - 64 for t in under) >= 3
    # the q chain's carry stops after each limb once
    low = [xs.low_ones(xs.device_x25519(k, u)[1]) for name, _, u in cases if name == "low-limbs-ones"]
    assert sorted(low) == list(range(1, 10))


def test_libsodium_edge_fixture():
    """the steered cases as an implementation independent of the reference and the oracle computes
    them; the fixture holds exactly the cases steered_cases builds today"""
    edges = xs.load_edges()
    steered = [(k.hex(), u.hex(), t.to_bytes(32, "little").hex(), name)
               for k in xs.SCALARS for name, t, u in xs.steered_cases(k)]
    assert [(e["k"], e["u"], e["out"], e["class"]) for e in edges if e["class"] in xs.CLASSES] == steered
    for e in edges:
        k, u = bytes.fromhex(e["k"]), bytes.fromhex(e["u"])
        assert xs.x25519_ref(k, u).hex() == e["out"] and or_x25519(k, u).hex() == e["out"], e["class"]
        if e["class"] not in xs.CLASSES:         # the steered ones go through the restatement above
            assert xs.device_x25519(k, u)[0].hex() == e["out"], e["class"]


# ---- fe_from_words ---------------------------------------------------------------------------------
def test_from_words_every_bit():
    """u = 2^i and its complement in 255 bits (mod 2^256: all ones for i = 255) for every bit i:
    each bit lands in its limb, bit 255 is dropped, and the ladder on it matches the reference"""
    k = xs.SCALARS[1]
    for i in range(256):
        for u in (1 << i, ((1 << 255) - 1 - (1 << i)) % (1 << 256)):
            w = [u >> (32 * j) & (U32 - 1) for j in range(8)]
            f = xs.fe_from_words(w)
            assert all(x <= m for x, m in zip(f, MASK)) and xs.limbs_value(f) == u & ((1 << 255) - 1), i
            got, br = xs.device_x25519(k, _b(u))
            assert got == xs.x25519_ref(k, _b(u)), (i, hex(u))
            assert not br["pass2_changed"]


# ---- fe_to_words on hand-built limbs -----------------------------------------------------------
def _to_int(f, **kw):
    w, br = xs.fe_to_words(f, **kw)
    return int.from_bytes(_words(w), "little"), br


def test_low_order_points_hand_p_to_to_words():
    """A low-order u ends the ladder at z2 = 0 mod p, and the product x2 * z2^(p-2) arrives at
    fe_to_words not as 0 but as its other representative, p itself: q = 1, and the output is 0 only
    because p is subtracted.  So the low-order inputs are what tells the seed `+ 19u` of q from
    `+ 18u` (which would let p through as it stands)."""
    for k in (xs.SCALARS[0], bytes(range(32))):
        for v in (0, 1, P - 1, P, P + 1) + xs.ORDER8:
            r = xs.device_ladder(k, _b(v))
            assert xs.limbs_value(r) == P, hex(v)
            got, br = _to_int(r)
            assert got == 0 and br["q"] == 1
            assert _to_int(r, q_seed=18)[0] == P


def test_to_words_at_p_on_hand_built_limbs():
    """The outputs p - 1 and 1 (= p + 1) are x-coordinates of low-order points, which no clamped
    scalar reaches (a multiple of 8 takes every point into a prime-order subgroup), so the ladder
    never hands p - 1 or p + 1 to fe_to_words and the mutant `+ 20u` of the seed of q is equivalent
    on every input the kernel can see.  It is told apart here, on the restated fe_to_words with
    hand-built limbs, along with the other values around p."""
    for v in (0, 1, 18, 19, P - 2, P - 1, P, P + 1, P + 18, (1 << 255) - 1):
        got, br = _to_int(xs.value_limbs(v))
        assert got == v % P and br["q"] == (v >= P), v
    assert _to_int(xs.value_limbs(P), q_seed=18)[0] != 0                 # q stays 0: p comes out as p
    assert _to_int(xs.value_limbs(P - 1), q_seed=20)[0] != P - 1         # q = 1 one too early
    assert _to_int(xs.value_limbs(P + 1), q_mul=1)[0] != 1               # 19u * q -> q
    # values >= 2^255 as fe_carry leaves them: limbs 2..9 all ones under a limb 1 of 2^25 + x
    for x, y in itertools.product((0, 1, 5, 1 << 17), (0, 1, M26 - 19, M26 - 18, M26)):
        f = [y, (1 << 25) + x] + list(MASK[2:])
        got, br = _to_int(f)
        assert br["ge_2_255"] and br["c9"] == 1 and br["wrap0"] == (y >= M26 - 18)
        assert got == xs.limbs_value(f) % P, (x, y)


# ---- bounds: a fixed point of interval arithmetic ----------------------------------------------------
class Bounds:
    """The field operations on worst-case upper bounds per limb (lower bound 0).  Every operation
    is monotone in its inputs -- sums, products, shifts, and x & mask <= min(x, mask) -- so running
    it on upper bounds gives upper bounds.  Asserts what the header comment of cz_x25519.hip claims
    and what each instruction's width needs; keeps the largest figures it saw."""
    top = {"mul_in": 0, "column": 0, "sub_g1": 0, "carry_limb1": 0}

    @classmethod
    def carry(cls, h, width):
        h, out = list(h), [0] * 10
        for i in range(9):
            out[i] = min(h[i], MASK[i])
            h[i + 1] += h[i] >> LW[i]
            assert h[i + 1] < width
        out[9] = min(h[9], M25)
        h0 = out[0] + 19 * (h[9] >> 25)
        assert h0 < width
        out[0] = min(h0, M26)
        out[1] += h0 >> 26
        assert max(out) < U32
        return out

    @classmethod
    def add(cls, f, g):
        h = [a + b for a, b in zip(f, g)]
        assert max(h) < U32
        return h

    @classmethod
    def sub(cls, f, g):
        # f >= 0: never negative iff g <= the limb of 2p, for a limb 1 as large as fe_carry leaves it
        assert all(b <= p2 for b, p2 in zip(g, P2)), g
        cls.top["sub_g1"] = max(cls.top["sub_g1"], g[1])
        return cls.carry([a + p2 for a, p2 in zip(f, P2)], U32)

    @classmethod
    def mul(cls, f, g):
        assert max(f) < 1 << 27 and max(g) < 1 << 27                     # "inputs to mul are kept below 2^27"
        assert 19 * max(g) < U32 and 19 * max(f) < U32 and 2 * max(f) < U32
        cls.top["mul_in"] = max(cls.top["mul_in"], max(f), max(g))
        h = [0] * 10
        for i in range(10):
            for j in range(10):
                h[(i + j) % 10] += f[i] * g[j] * (2 if i & 1 and j & 1 else 1) * (19 if i + j >= 10 else 1)
        assert max(h) < 1 << 63                                            # "each column stays below 2^63"
        cls.top["column"] = max(cls.top["column"], max(h))
        out = cls.carry(h, U64)
        cls.top["carry_limb1"] = max(cls.top["carry_limb1"], out[1])
        return out

    @classmethod
    def sq(cls, f):
        return cls.mul(f, f)             # the same columns, the symmetric terms taken once and doubled

    @classmethod
    def mul_small(cls, f, k):
        assert k * max(f) < U64
        return cls.carry([x * k for x in f], U64)


def _join(a, b):
    return [max(x, y) for x, y in zip(a, b)]


def _fixed_point():
    """Bounds of (x2, z2, x3, z3) that one more ladder step does not grow, then of the inverse and
    of the product handed to fe_to_words.  The swaps mix x2 with x3 and z2 with z3, so each pair
    shares the larger bound."""
    one = [1] + [0] * 9
    x1 = list(MASK)                                                        # fe_from_words masks every limb
    x, z = _join(one, x1), _join([0] * 10, one)
    for rounds in range(1, 20):
        x2, z2, x3, z3 = xs.ladder_step(x1, x, z, x, z, Bounds)
        nx, nz = _join(x, _join(x2, x3)), _join(z, _join(z2, z3))
        if (nx, nz) == (x, z):
            break
        x, z = nx, nz
    else:
        raise AssertionError("the bounds keep growing")
    r = Bounds.mul(x, xs.fe_invert(z, Bounds))
    return rounds, x, z, r


def test_limb_bounds_hold_at_the_fixed_point():
    rounds, x, z, r = _fixed_point()
    assert rounds <= 4
    # the figures the header comment speaks of, at their worst
    assert Bounds.top["mul_in"] < 1 << 27
    assert Bounds.top["column"] < 1 << 63
    assert M25 < Bounds.top["sub_g1"] <= P2[1]          # fe_sub takes a limb 1 above its mask, and has room for it
    # a carried element: every limb within its width but limb 1, which keeps fe_carry's last carry
    for f in (x, z, r):
        assert all(f[i] <= MASK[i] for i in range(10) if i != 1) and M25 < f[1] < (1 << 25) + (1 << 20)
    # the bounds are reached in order of magnitude: restated values come close to them
    k, u = xs.SCALARS[0], xs.steered_cases(xs.SCALARS[0])[0][2]
    assert max(xs.device_ladder(k, u)) <= max(r)


def test_second_carry_pass_of_to_words_is_dead():
    """fe_to_words runs fe_carry32 twice.  The second pass changes a limb only when the first leaves
    limb 1 = 2^25: limb 1 = 2^25 - 1 after masking, plus the carry of the wrapped 19 out of limb 0.
    That carry needs a ripple out of limb 9, which needs limb 1 >= 2^25 going in, so limb 1 was
    2^26 - 1 (it is below 2^26).  fe_carry leaves limb 1 <= 2^25 - 1 + c with c = (h0 + 19 (h9 >> 25))
    >> 26 < 2^20 at the worst-case columns of the fixed point above: far below 2^26 - 1.  So for
    everything the kernel hands to fe_to_words the second pass is the identity, and limb 1 never
    enters the q chain as 2^25.  Shown on the extremes of that range; just outside it (limb 1 =
    2^26 - 1) the pass does its work and the result is still right, which is what it is there for."""
    r1 = _fixed_point()[3][1]
    assert r1 < M26                                      # the bound of the proof
    limb0 = (0, 1, M26 - 19, M26 - 18, M26)
    limb1 = (0, 1, M25 - 1, M25, 1 << 25, (1 << 25) + 1, r1 - 1, r1)
    highs = [tuple(m - b for m, b in zip(MASK[2:], bits)) for bits in itertools.product((0, 1), repeat=8)]
    highs.append((0,) * 8)
    for a, b, hi in itertools.product(limb0, limb1, highs):
        f = [a, b] + list(hi)
        got, br = _to_int(f)
        assert not br["pass2_changed"] and not br["limb1_2_25"], f
        assert got == xs.limbs_value(f) % P, f
    for a in (M26 - 18, M26):
        f = [a, M26] + list(MASK[2:])
        got, br = _to_int(f)
        assert br["pass2_changed"] and got == xs.limbs_value(f) % P
