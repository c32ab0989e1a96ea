"""The device's radix-2^26 arithmetic mod 2^130 - 5 (cz_device.h f26_from32, f26_mul, f26_add,
f26_pow, f26_to32, and combine_tag's Horner in cz_kernels.hip) restated with Python integers.

These helpers join the Poly1305 partials of a segmented frame (combine_tag) and of the one-launch
box's threads (k_nacl_one).  Every intermediate is checked against the bound its u32 / u64
instruction assumes (limbs below 2^27 on input, 5 * b below 2^32, product columns below 2^64, the
unmasked limb 1 that f26_mul / f26_add leave, limb 1 below 2^26 where f26_to32 packs it) and every
value against big integers mod p, over all-max limbs, h4 = 4, powers of r up to 2^15, long add /
mul chains and random inputs.  The last tests build, constructively, partials that make f26_to32
take the carry out of limb 4 (`l0 += c * 5`): the GPU edge tests run the same inputs.
"""
import random

import pytest

import poly_steer as ps

P = ps.P
M26 = (1 << 26) - 1
M32 = (1 << 32) - 1
U32, U64 = 1 << 32, 1 << 64


def f26_value(a):
    return sum(x << (26 * i) for i, x in enumerate(a))


def f26_from32(h0, h1, h2, h3, h4):
    assert max(h0, h1, h2, h3) <= M32 and (h4 << 24) < U32
    return (h0 & M26, ((h0 >> 26) | (h1 << 6)) & M26, ((h1 >> 20) | (h2 << 12)) & M26,
            ((h2 >> 14) | (h3 << 18)) & M26, (h3 >> 8) | (h4 << 24))


def f26_mul(a, b):
    assert max(a) < 1 << 27 and max(b) < 1 << 27  # the documented input range
    s = [x * 5 for x in b]
    assert max(s) < U32  # u32 multiply
    d = [a[0] * b[0] + a[1] * s[4] + a[2] * s[3] + a[3] * s[2] + a[4] * s[1],
         a[0] * b[1] + a[1] * b[0] + a[2] * s[4] + a[3] * s[3] + a[4] * s[2],
         a[0] * b[2] + a[1] * b[1] + a[2] * b[0] + a[3] * s[4] + a[4] * s[3],
         a[0] * b[3] + a[1] * b[2] + a[2] * b[1] + a[3] * b[0] + a[4] * s[4],
         a[0] * b[4] + a[1] * b[3] + a[2] * b[2] + a[3] * b[1] + a[4] * b[0]]
    r = [0] * 5
    for i in range(4):
        assert d[i] < U64
        d[i + 1] += d[i] >> 26
        r[i] = d[i] & M26
    assert d[4] < U64
    c = d[4] >> 26
    r[4] = d[4] & M26
    t = r[0] + c * 5
    assert t < U64
    r[0] = t & M26
    r[1] += t >> 26
    assert r[1] < (1 << 26) + (1 << 7)  # limb 1 is left unmasked (the bound cz_device.h documents)
    assert f26_value(r) % P == f26_value(a) * f26_value(b) % P
    return tuple(r)


def f26_add(a, b):
    r, c = [0] * 5, 0
    for i in range(5):
        v = a[i] + b[i] + c
        assert v < U32
        r[i] = v & M26
        c = v >> 26
    t = r[0] + c * 5
    assert t < U32
    r[0] = t & M26
    r[1] += t >> 26
    assert r[1] <= 1 << 26
    assert f26_value(r) % P == (f26_value(a) + f26_value(b)) % P
    return tuple(r)


def f26_pow(r, e):
    if e == 0:
        return (1, 0, 0, 0, 0)
    acc = base = r
    have, bit = False, 0
    while e >> bit:
        if bit:
            base = f26_mul(base, base)
        if (e >> bit) & 1:
            acc = f26_mul(acc, base) if have else base
            have = True
        bit += 1
    return acc


def f26_to32(a, trace=None):
    l0, l1, l2, l3, l4 = a
    assert max(a) < U32
    c = l1 >> 26; l1 &= M26
    l2 += c; c = l2 >> 26; l2 &= M26
    l3 += c; c = l3 >> 26; l3 &= M26
    l4 += c; c = l4 >> 26; l4 &= M26
    if trace is not None:
        trace.append(c)
    l0 += c * 5; c = l0 >> 26; l0 &= M26
    l1 += c
    # the packing ORs shifted limbs together and `l1 << 26` is a u32: limb 1 must fit 26 bits
    assert l1 <= M26, "f26_to32 would drop bit 26 of limb 1"
    h = (l0 | (l1 << 26) & M32, (l1 >> 6) | (l2 << 20) & M32, (l2 >> 12) | (l3 << 14) & M32,
         (l3 >> 18) | (l4 << 8) & M32, l4 >> 24)
    assert h[4] <= 3  # poly_finish folds nothing after a combine
    assert ps.limbs_value(h) % P == f26_value(a) % P
    return h


def combine(recs, r_limbs, trace=None):
    """combine_tag's Horner: recs = [(h0..h4, m)] per segment, r_limbs = the clamped r words"""
    r = f26_from32(*r_limbs, 0)
    H = f26_from32(*recs[0][0])
    n = len(recs)
    if n > 1:
        m_last = recs[-1][1]
        m_mid = recs[1][1] if n > 2 else m_last
        base, pm, pl, bit = r, (1, 0, 0, 0, 0), (1, 0, 0, 0, 0), 0
        while (m_mid | m_last) >> bit:
            if bit:
                base = f26_mul(base, base)
            if (m_mid >> bit) & 1:
                pm = f26_mul(pm, base)
            if (m_last >> bit) & 1:
                pl = f26_mul(pl, base)
            bit += 1
        for s in range(1, n - 1):
            h, m = recs[s]
            H = f26_add(f26_mul(H, pm if m == m_mid else f26_pow(r, m)), f26_from32(*h))
        H = f26_add(f26_mul(H, pl), f26_from32(*recs[-1][0]))
    else:
        return recs[0][0]   # one record: finished as it stands, no radix-2^26 round trip
    return f26_to32(H, trace)


def _r_limbs(rv):
    return tuple(rv >> (32 * i) & M32 for i in range(4))


R_MAX = ps.R_MASK
ALL_ONES_H = (M32, M32, M32, M32, 4)   # above anything poly_block leaves (h4 = 4 comes with h3 < 2^31 + 1)


def test_from32_to32_round_trip_at_the_extremes():
    rng = random.Random(26)
    cases = [(0, 0, 0, 0, 0), (M32, M32, M32, M32, 3), (M32 - 4, M32, M32, M32, 3), (M32, M32, M32, M32, 0)]
    cases += [tuple(rng.getrandbits(32) for _ in range(4)) + (rng.randrange(4),) for _ in range(500)]
    for h in cases:
        a = f26_from32(*h)
        assert max(a) < 1 << 26 and f26_value(a) == ps.limbs_value(h)
        assert f26_to32(a) == h
    for h in (ALL_ONES_H, (0, 0, 0, 0, 4)):
        a = f26_from32(*h)
        assert max(a) < 1 << 27 and f26_value(a) == ps.limbs_value(h)


def test_to32_takes_add_results_only_one_segment_records_bypass_it():
    """f26_to32 packs with ORs and a u32 `l1 << 26`, so limb 1 must end below 2^26.  After f26_add
    it does (a carry out of limb 4 needs limb 1 = 2^26, which the first step clears).  Straight
    from f26_from32 it need not: a record with h4 = 4 has l[4] >= 2^26, carries out, and `l0 += 5`
    can ripple into an all-ones limb 1.  The device holds the residue 2^53 + e as
    2^130 + 2^53 - 5 + e: limb 0 = 2^26 - 5 + e, limb 1 all ones, limb 2 odd -- the OR then loses
    the carry into limb 2.  combine_tag used to send a one-segment frame's record through this
    round trip; it now finishes such a record as it stands (restated in combine())."""
    rng = random.Random(53)
    key = rng.randbytes(32)
    for e in range(5):
        msg = ps.steer(key, 64, (1 << 53) + e, rng)
        h = ps.device_state(msg, key)
        assert h == (((1 << 53) - 5 + e) & M32, ((1 << 53) - 5 + e) >> 32, 0, 0, 4)
        with pytest.raises(AssertionError, match="bit 26 of limb 1"):
            f26_to32(f26_from32(*h))
        assert combine([(h, 4)], _r_limbs(ps.key_r(key))) == h
        assert ps.device_finish(h, ps.key_s(key))[0] == ps.poly1305(msg, key)


def test_mul_add_bounds_at_all_max_limbs():
    top = ((1 << 27) - 1,) * 5           # the documented input bound, every limb
    f26_mul(top, top)
    mx = f26_from32(*ALL_ONES_H)
    a = f26_mul(mx, mx)
    for _ in range(200):                # chained: limb 1 never grows past a valid input
        a = f26_add(f26_mul(a, mx), mx)
        a = f26_add(a, a)
    f26_to32(a)


def test_pow_against_big_integers():
    rng = random.Random(15)
    rs = [R_MAX, 1, 2, 4 << 32, 1 << 124, 0] + [rng.getrandbits(128) & ps.R_MASK for _ in range(6)]
    rs += [0x0FFFFFFC << (32 * i) for i in range(1, 4)] + [0x0FFFFFFF]
    es = sorted(set(list(range(0, 70)) + [2 ** k + d for k in range(6, 16) for d in (-1, 0, 1)] + [4 * 6, 4 * 128]))
    for rv in rs:
        r = f26_from32(*_r_limbs(rv), 0)
        for e in es:
            assert f26_value(f26_pow(r, e)) % P == pow(rv, e, P), (hex(rv), e)


def test_long_random_chains():
    rng = random.Random(2626)
    for trial in range(200):
        rv = rng.getrandbits(128) & ps.R_MASK if trial % 4 else R_MAX
        r = f26_from32(*_r_limbs(rv), 0)
        H, ref = f26_from32(*ALL_ONES_H), ps.limbs_value(ALL_ONES_H)
        for step in range(40):
            h = ALL_ONES_H if (trial + step) % 7 == 0 else \
                tuple(rng.getrandbits(32) for _ in range(4)) + (rng.randrange(5),)
            e = rng.choice([1, 2, 4, 24, 255, 256, 512, 32768])
            H = f26_add(f26_mul(H, f26_pow(r, e)), f26_from32(*h))
            ref = (ref * pow(rv, e, P) + ps.limbs_value(h)) % P
            assert f26_value(H) % P == ref
        assert ps.limbs_value(f26_to32(H)) % P == ref


def _device_recs(key, pieces):
    """the partial records the segment kernels write: each piece's limbs from zero and block count"""
    return [(ps.device_state(p, key), (len(p) + 15) // 16) for p in pieces]


@pytest.mark.parametrize("nseg,mid", [(2, None), (3, None), (4, None), (4, 80)])
def test_combine_matches_poly1305_with_steered_partials(nseg, mid):
    """combine_tag's Horner over records whose partials sit on the edge residues (all limbs ones,
    zero, the h4 boundaries), equal middle segments and one middle segment of another length (its
    own f26_pow), the joined value at every final target"""
    rng = random.Random(nseg * 100 + (mid or 0))
    for key in [rng.randbytes(32) for _ in range(3)]:
        s = ps.key_s(key)
        for j, (name, f) in enumerate(ps.TARGETS):
            lens = [32] + [64] * (nseg - 2) + [64 + 16 * (j % 3) + j % 16]
            if mid:
                lens[1] = mid
            parts = [ps.PARTIALS[(j + i) % len(ps.PARTIALS)] for i in range(nseg - 1)]
            msg = ps.steer_pieces(key, lens, parts, f(s), rng, head=b"\x02")
            pieces, o = [], 0
            for n in lens:
                pieces.append(msg[o:o + n])
                o += n
            h = combine(_device_recs(key, pieces), _r_limbs(ps.key_r(key)))
            assert ps.limbs_value(h) % P == f(s) % P, name
            assert ps.device_finish(h, s)[0] == ps.poly1305(msg, key), name


def test_to32_carry_out_of_limb_4_constructed():
    """f26_to32's `l0 += c * 5` runs only when the joined value is 2^131 - k, k = 1..5, before
    reduction: the last f26_add must see a = 2^130 - y - k from f26_mul and b = 2^130 + y from a
    partial the device holds with h4 = 4.  poly_steer.steer_carry_out builds exactly that (the last
    segment's partial at a residue T the device holds as T + p, the whole message at 10 - k); a
    search over random and edge partials finds none (it needs 2^-126 luck), so the construction is
    what the GPU tests run.  The carried-out value packs correctly because limb 1 is then zero."""
    rng = random.Random(131)
    found = 0
    for key in [rng.randbytes(32) for _ in range(4)]:
        s = ps.key_s(key)
        for k in range(1, 6):
            for lens in ([32, 64], [32, 64, 64 + 7], [96, 32, 256, 48]):
                msg, pieces = ps.steer_carry_out(key, lens, k, rng, head=b"\x01")
                trace = []
                h = combine(_device_recs(key, pieces), _r_limbs(ps.key_r(key)), trace)
                assert trace == [1], "the constructed partials must take the carry-out"
                assert ps.limbs_value(h) == 10 - k
                assert ps.device_finish(h, s)[0] == ps.poly1305(msg, key)
                found += 1
    assert found == 60


def test_to32_carry_out_search_over_edge_partials():
    """The search the construction stands in for: pairs and triples of edge partials (h4 = 0..4 with
    all-ones, zero and boundary limbs) and random ones under edge and random r.  The carry-out
    shows where partials near 2^130 are simply added (r = 1, or a zero partial in front; 2^130 - 1
    is how the device holds the residue 4).  Wherever it happens the packed value is right and limb
    1 fits 26 bits (asserted in f26_to32)."""
    rng = random.Random(7)
    edge = [(M32, M32, M32, M32, 3), (M32 - 4, M32, M32, M32, 3), (0, 0, 0, 0, 4), (M32, M32, M32, 1 << 31, 4),
            (0, 0, 0, 0, 0), (M32, M32, M32, M32, 0), (5, 0, 0, 0, 4), (M32 - 5, M32, M32, M32, 3)]
    edge += [tuple(rng.getrandbits(32) for _ in range(4)) + (rng.randrange(4),) for _ in range(8)]
    carried = {}
    for rv in [R_MAX, 1, 2, 1 << 124] + [rng.getrandbits(128) & ps.R_MASK for _ in range(4)]:
        trace = []
        for a in edge:
            for b in edge:
                for m in (1, 4, 6, 255):
                    combine([(a, 2), (b, m)], _r_limbs(rv), trace)
                    combine([(a, 2), (b, m), (a, m)], _r_limbs(rv), trace)
        carried[rv] = sum(trace)
    assert carried[1] > 0
