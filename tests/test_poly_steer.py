"""The oracle's Poly1305 and secretbox at the reduction and carry edges, on steered inputs.

The GPU suites are pinned to the oracle (oracle/curve_oracle.c), whose own Poly1305 is checked on
libsodium vectors of ordinary messages only.  poly_steer.py builds messages whose final accumulator
is any chosen residue, so here every edge target (the freeze at 0..6 and p-1..p-6, the h4
boundaries, all-ones carry chains in the +5, fold and pad additions) is put through or_poly1305
and or_box_afternm and compared with a big-integer Poly1305, bit for bit.  The same inputs go to
the compiled kernels in test_gpu_poly_edges.py; this file proves on the CPU that they exist and
that the restated device arithmetic (test_poly_radix32.poly_block + poly_steer.device_finish)
takes its rare branches on them.
"""
import random

import pytest

import poly_steer as ps
from cz_testlib import or_box_afternm, or_box_open_afternm, or_poly1305

MAC_LENS = [32, 33, 47, 48, 63, 64, 95, 4097]


def _keys(seed, n=8):
    rng = random.Random(seed)
    return [rng.randbytes(32) for _ in range(n)]


@pytest.mark.parametrize("nbytes", MAC_LENS)
def test_oracle_poly1305_at_steered_targets(nbytes):
    rng = random.Random(1305 + nbytes)
    for key in _keys(nbytes):
        s = ps.key_s(key)
        for name, f in ps.TARGETS:
            T = f(s)
            msg = ps.steer(key, nbytes, T, rng, head=rng.randbytes(1))
            assert ps.accumulate(msg, key) == T % ps.P, name
            want = ps.poly1305(msg, key)
            assert or_poly1305(msg, key) == want, f"{name} at {nbytes} bytes"
            # the device arithmetic restated agrees too (and checks its bounds on the way)
            tag, _ = ps.device_finish(ps.device_state(msg, key), s)
            assert tag == want, f"{name} at {nbytes} bytes (restated device arithmetic)"


@pytest.mark.parametrize("nbytes", MAC_LENS)
def test_oracle_box_chosen_key_at_steered_targets(nbytes):
    """crypto_box_afternm with m[0:32] != 0 keys the MAC with c[0:32]: m = keystream ^ (K32 || M)
    makes the oracle compute Poly1305(K32, M) for a key and a message of our choosing"""
    rng = random.Random(2610 + nbytes)
    k, n24 = rng.randbytes(32), rng.randbytes(24)
    for key32 in _keys(77 + nbytes):
        s = ps.key_s(key32)
        for name, f in ps.TARGETS:
            msg = ps.steer(key32, nbytes, f(s), rng)
            rc, c = or_box_afternm(ps.chosen_key_box(k, n24, key32, msg), n24, k)
            assert rc == 0 and c[:16] == bytes(16) and c[32:] == msg
            assert c[16:32] == ps.poly1305(msg, key32), f"{name} at {nbytes} bytes"


def test_oracle_open_at_tag_zero_and_ones():
    """The open's tag comparison on the all-zero and all-ones tags: accepted as sealed, rejected with
    any one bit of the tag flipped"""
    rng = random.Random(99)
    k, n24 = rng.randbytes(32), rng.randbytes(24)
    key = ps.box_keystream(k, n24, 32)
    for idx, tagv in ((ps.TAG_ZERO, bytes(16)), (ps.TAG_ONES, b"\xff" * 16)):
        msg = ps.steer(key, 100, ps.TARGETS[idx][1](ps.key_s(key)), rng)
        assert ps.poly1305(msg, key) == tagv
        c = bytes(16) + tagv + msg
        rc, m = or_box_open_afternm(c, n24, k)
        assert rc == 0 and m[:32] == bytes(32)
        for bit in range(128):
            bad = bytearray(c)
            bad[16 + bit // 8] ^= 1 << (bit % 8)
            assert or_box_open_afternm(bytes(bad), n24, k)[0] == -1, bit


def test_targets_reach_the_rare_branches_of_the_device_arithmetic():
    """What the steered targets are for: on the restated device arithmetic each rare path of
    poly_finish is taken by some target -- p subtracted (ge) with the +5 carry crossing all four
    limbs, the h4 >= 4 fold with its carry crossing 0, 1, 2 and 3 limbs, every pad-add carry
    pattern -- and poly_block's h + m chain carries through all-ones limbs into h4."""
    rng = random.Random(4)
    seen = {"ge": set(), "fold_ripple": set(), "g_ripple": set(), "pad_carry": set(), "h4": set()}
    for key in _keys(5, 4):
        s = ps.key_s(key)
        for name, f in ps.TARGETS:
            msg = ps.steer(key, 48, f(s), rng)
            h = ps.device_state(msg, key)
            tag, br = ps.device_finish(h, s)
            assert tag == ps.poly1305(msg, key)
            assert br["fold_h4"] == 0  # see test_fold_never_carries_into_h4
            seen["ge"].add(br["ge"])
            seen["h4"].add(h[4])
            seen["g_ripple"].add(br["g_ripple"])
            seen["pad_carry"].add(br["pad_carry"])
            if br["fold"]:
                seen["fold_ripple"].add(br["fold_ripple"])
        for x in (0, 3):
            msg = ps.hm_ripple(key, 64, x, rng)
            before, after = ps.device_state(msg[:48], key), ps.device_state(msg, key)
            assert before[4] == 0 and before[1:4] == (ps.M32,) * 3 and before[0] == ps.M32 - x
            assert ps.limbs_value(after) % ps.P == ps.accumulate(msg, key)
            assert or_poly1305(msg, key) == ps.poly1305(msg, key)
    assert seen["ge"] == {False, True}
    assert seen["h4"] == {0, 1, 2, 3, 4}
    assert 4 in seen["g_ripple"]
    assert seen["fold_ripple"] >= {0, 1, 2, 3}
    assert seen["pad_carry"] >= {(0, 0, 0), (1, 1, 1), (0, 1, 1), (0, 0, 1)}


def test_fold_never_carries_into_h4():
    """poly_finish adds the first fold's carry into h4 (`h4 += carry`).  No accumulator the kernels
    produce takes it: it needs h4 = 4 with limbs >= 2^128 - 5.  poly_block leaves h4 = 4 only as
    (x & 3) = 3 plus the carry of its one chain, whose top column is lo(d3) + hi(d2) + carry with
    hi(d2) < 2^31 (d2 is five products of a limb < 2^32 and a multiplier < 1.25 * 2^28), so the
    limb it leaves is below 2^31 + 1; and f26_to32 masks l4 to 26 bits, so its h4 is at most 3 and
    nothing is folded.  Checked here at the extremes of the restated block step."""
    ones = (ps.M32,) * 4
    rmax = (0x0FFFFFFF, 0x0FFFFFFC, 0x0FFFFFFC, 0x0FFFFFFC)
    smax = [x + (x >> 2) for x in rmax]
    assert ps.M32 * (rmax[2] + rmax[1] + rmax[0] + smax[3]) + 6 * smax[2] < 1 << 63   # hi(d2) < 2^31
    rng = random.Random(8)
    top = 0
    for trial in range(2000):
        r = rmax if trial % 2 else tuple(rng.getrandbits(32) & m for m in rmax)
        h = (0, 0, 0, 0, 0)
        for b in range(6):
            m = ones if (trial + b) % 3 == 0 else tuple(rng.getrandbits(32) for _ in range(4))
            h = ps.device_poly_block(h, r, m, 1)
            if h[4] == 4:
                top = max(top, h[3])
                assert h[3] <= 1 << 31
    assert top > 0  # h4 = 4 was reached
