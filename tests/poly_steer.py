"""Steered Poly1305 inputs: messages whose accumulator ends at a chosen residue mod 2^130 - 5.

Poly1305 is h_n = (h_{n-1} + c_n + 2^128) * r mod p.  For a known non-zero r any target T of the
final accumulator is reached by solving one full 16-byte block, v = T * r^-1 - h_{n-1} mod p,
which is a valid block when it lies in [2^128, 2^129): about 1/4 of random prefixes, so the bytes
before it are redrawn until it does.  A trailing partial block is undone first.  This puts the
branches a random message takes with probability ~2^-100 (the conditional subtraction of p, the
h4 folds, all-ones carry chains) under the compiled kernels and the oracle; the reference is the
big-integer poly1305() below.  Helper module of test_poly_steer.py and test_gpu_poly_edges.py.
"""
from cz_testlib import or_hsalsa20, or_salsa20_stream
from test_poly_radix32 import poly_block as device_poly_block

P = (1 << 130) - 5
M32 = (1 << 32) - 1
M128 = (1 << 128) - 1
R_MASK = 0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF
PREFIX = (b"CurveZMQMESSAGEC", b"CurveZMQMESSAGES")
MAX_DRAWS = 64  # a draw succeeds with probability ~1/4: (3/4)^64 ~ 1e-8


def key_r(key):
    return int.from_bytes(key[:16], "little") & R_MASK


def key_s(key):
    return int.from_bytes(key[16:32], "little")


def block_values(msg):
    """The integers Poly1305 adds per 16-byte block (2^128, or the 0x01 byte after a partial block)"""
    for o in range(0, len(msg), 16):
        b = msg[o:o + 16]
        yield int.from_bytes(b, "little") | 1 << (8 * len(b))


def accumulate(msg, key, h=0):
    """The accumulator (a residue mod p) after `msg`, starting from h"""
    r = key_r(key)
    for v in block_values(msg):
        h = (h + v) * r % P
    return h


def poly1305(msg, key):
    """Big-integer Poly1305: the high-precision reference"""
    return ((accumulate(msg, key) + key_s(key)) & M128).to_bytes(16, "little")


def device_state(msg, key, h=(0, 0, 0, 0, 0)):
    """The partially reduced limbs (h0..h3, h4) the device's radix-2^32 poly_block holds after `msg`
    (the restatement in test_poly_radix32.py, which checks every instruction's bound as it goes)"""
    rv = key_r(key)
    r = tuple(rv >> (32 * i) & M32 for i in range(4))
    for o in range(0, len(msg), 16):
        b = msg[o:o + 16]
        v = int.from_bytes(b, "little") | (1 << (8 * len(b)) if len(b) < 16 else 0)
        h = device_poly_block(h, r, tuple(v >> (32 * i) & M32 for i in range(4)), 1 if len(b) == 16 else 0)
    return h


def limbs_value(h):
    return h[0] | h[1] << 32 | h[2] << 64 | h[3] << 96 | h[4] << 128


def steer_from(key, h0, nbytes, T, rng, head=b"", accept=None, draws=MAX_DRAWS):
    """`nbytes` message bytes that take the accumulator from h0 to T (mod p): `head` first (kept as
    given), random bytes, the solved block as the last full block, then a random partial block.
    Needs two full blocks, at least one of them outside `head`.  accept(msg): a further condition to
    redraw on (e.g. on the device's representation).  Raises after `draws` draws; never gives up
    silently."""
    r = key_r(key)
    if r == 0:
        raise ValueError("r = 0 cannot be steered")
    nfull, rem = divmod(nbytes, 16)
    if nfull < 2 or len(head) > 16 * (nfull - 1) - 1:
        raise ValueError("steering needs a free block before the solved one")
    rinv = pow(r, -1, P)
    T %= P
    # drawn once: everything before the last 17 full blocks; the 16 before the solved one are
    # redrawn, so that under r = 1, 2, ... (where the accumulator is nearly a plain sum of the
    # blocks, and 16 of them spread evenly around p) the draws still cover every residue
    fixed = 16 * max(0, nfull - 17)
    bulk = head + rng.randbytes(max(0, fixed - len(head)))
    hb = accumulate(bulk[:fixed], key, h0)
    for _ in range(draws):
        free = bulk[fixed:] + rng.randbytes(16 * (nfull - 1) - max(fixed, len(bulk)))
        tail = rng.randbytes(rem)
        want = T
        if rem:
            want = (T * rinv - (int.from_bytes(tail, "little") | 1 << (8 * rem))) % P
        v = (want * rinv - accumulate(free, key, hb)) % P
        if v >> 128 != 1:
            continue
        msg = bulk[:fixed] + free + (v & M128).to_bytes(16, "little") + tail
        assert len(msg) == nbytes and msg.startswith(head)
        assert accumulate(msg, key, h0) == T
        if accept is None or accept(msg):
            return msg
    raise RuntimeError(f"no steered message in {draws} draws")


def steer(key, nbytes, T, rng, head=b"", accept=None, draws=MAX_DRAWS):
    """A message of nbytes whose Poly1305 accumulator under `key` ends at T"""
    return steer_from(key, 0, nbytes, T, rng, head, accept, draws)


def steer_pieces(key, lens, partials, T, rng, head=b""):
    """A message cut into pieces of lens[i] bytes (multiples of 16 but the last): piece i's own
    Horner value from zero is steered to partials[i] (None: left random) where the piece has two
    full blocks and comes before the blocks that steer the whole message's accumulator to T -- the
    partial records of a segmented frame, or the per-thread partials of the one-launch box."""
    assert all(n % 16 == 0 for n in lens[:-1]) and sum(lens) >= 32
    k = len(lens)  # the trailing pieces that hold the two full blocks the final steer needs
    while k > 0 and sum(lens[k:]) // 16 < 2:
        k -= 1
    out = b""
    for i in range(k):
        hd = head if i == 0 else b""
        if partials[i] is not None and lens[i] >= 32 and len(hd) < lens[i] - 16:
            piece = steer_from(key, 0, lens[i], partials[i], rng, hd)
            assert accumulate(piece, key) == partials[i] % P
        else:
            piece = hd + rng.randbytes(lens[i] - len(hd))
        out += piece
    out += steer_from(key, accumulate(out, key), sum(lens[k:]), T, rng, head if k == 0 else b"")
    assert accumulate(out, key) == T % P
    return out


# ---- keys ------------------------------------------------------------------------------------
def message_keystream(precom, direction, counter, nbytes):
    """The XSalsa20 keystream of a MESSAGE box (nonce = "CurveZMQMESSAGE{C|S}" + BE64(counter)):
    bytes 0..31 are the Poly1305 key r || s, byte 32 covers the flags byte, 33.. the payload"""
    return or_salsa20_stream(nbytes, counter.to_bytes(8, "big"), 0, or_hsalsa20(PREFIX[direction], precom))


def box_keystream(k, n24, nbytes):
    return or_salsa20_stream(nbytes, n24[16:24], 0, or_hsalsa20(n24[:16], k))


def chosen_key_box(k, n24, key32, msg):
    """m for crypto_box_afternm / crypto_secretbox such that the MAC is Poly1305(key32, msg): NaCl keys
    the MAC with c[0:32] = keystream[0:32] ^ m[0:32], and c[32:] = msg"""
    want = key32 + msg
    ks = box_keystream(k, n24, len(want))
    return bytes(a ^ b for a, b in zip(ks, want))


# ---- targets ---------------------------------------------------------------------------------
def _pad_ripple(s, j):
    """limbs below j zero, limb j all ones (carries out when s_j >= 1), limbs above j the complement
    of s's: the carry ripples through every tag word above j"""
    sl = [s >> (32 * i) & M32 for i in range(4)]
    return sum((0 if i < j else M32 if i == j else M32 - sl[i]) << (32 * i) for i in range(4))


def targets():
    """(name, f(s) -> T): final-accumulator targets; s is the key's pad"""
    out = []
    for d in range(7):
        out.append((f"freeze+{d}", lambda s, d=d: d))
    for d in range(1, 7):
        out.append((f"freeze-p-{d}", lambda s, d=d: P - d))
    for k in (1, 2, 3):
        for d in (-1, 0, 1):
            out.append((f"h4-{k}*2^128{d:+d}", lambda s, k=k, d=d: (k << 128) + d))
    for k in (32, 64, 96, 128, 130):
        for d in (1, 5, 6):
            out.append((f"ripple-2^{k}-{d}", lambda s, k=k, d=d: (1 << k) - d))
    # the device holds a residue T < 2^96 as T + p = 2^130 + (T - 5): h4 = 4 and low limbs T - 5, so
    # these make poly_finish's first fold (+5) ripple a carry across limb 0, 0..1, 0..2
    for k in (32, 64, 96):
        for d in (0, 4):
            out.append((f"fold-2^{k}+{d}", lambda s, k=k, d=d: (1 << k) + d))
    out.append(("pad-tag-zero", lambda s: -s & M128))
    out.append(("pad-tag-ones", lambda s: (-s - 1) & M128))
    for j in range(3):
        out.append((f"pad-ripple-from-{j}", lambda s, j=j: _pad_ripple(s, j)))
    return out


TARGETS = targets()
TAG_ZERO = [n for n, _ in TARGETS].index("pad-tag-zero")
TAG_ONES = [n for n, _ in TARGETS].index("pad-tag-ones")
# partial-record targets of segments and threads: residues whose limbs are all ones / all zero and
# the h4 boundaries
PARTIALS = [P - 1, 0, 1 << 128, (1 << 128) - 1, 2 << 128, (3 << 128) - 1, (3 << 128) + 1, (1 << 130) - 6, 5]


def hm_ripple(key, nbytes, x, rng, head=b""):
    """The h + m carry chain with all-ones limbs: the accumulator before the last full block is
    steered to 2^128 - 1 - x and the last block's low word is x + 1 with every other word
    0xffffffff, so adding it ripples a carry through all four limbs into h4; the steered prefix
    holds that residue as it stands (limbs below 2^128, h4 = 0): the other representative, plus p,
    would be h4 = 4 over a top limb of all ones, which poly_block never leaves (h4 = 4 comes with
    h3 <= 2^31, test_poly_steer.test_fold_never_carries_into_h4).  Asserted on the restated
    device arithmetic."""
    want = (1 << 128) - 1 - x
    pre = nbytes // 16 * 16 - 16
    last = ((x + 1) | (M128 >> 32 << 32)).to_bytes(16, "little")
    msg = steer(key, pre, want, rng, head)
    assert limbs_value(device_state(msg, key)) == want
    return msg + last + rng.randbytes(nbytes % 16)


def device_finish(h, s):
    """cz_device.h poly_finish restated: (tag, branches) from the device's limbs and the pad.
    branches records what the rare paths did, so a test can tell that its inputs reached them:
    fold (the 5 * (h4 >> 2) added), fold_ripple (limbs the fold's carry crossed), fold_h4 (its carry
    into h4), ge (p subtracted), g_ripple (limbs the +5 carry crossed), pad_carry (carries out of
    tag words 0..2)."""
    h0, h1, h2, h3, h4 = h
    assert h4 <= 4 and all(x <= M32 for x in (h0, h1, h2, h3))
    c = (h4 >> 2) * 5
    h4 &= 3
    limbs, fold_ripple = [], 0
    for x in (h0, h1, h2, h3):
        t = x + c
        limbs.append(t & M32)
        c = t >> 32
        fold_ripple += c
    fold_h4 = c
    h4 += c
    g, c, g_ripple = [], 5, 0
    for x in limbs:
        t = x + c
        g.append(t & M32)
        c = t >> 32
        g_ripple += c
    ge = (h4 + c) >> 2 != 0
    if ge:
        limbs = g
    tag, c, pad_carry = 0, 0, []
    for i, x in enumerate(limbs):
        t = x + (s >> (32 * i) & M32) + c
        tag |= (t & M32) << (32 * i)
        c = t >> 32
        pad_carry.append(c)
    br = {"fold": h[4] >> 2, "fold_ripple": fold_ripple, "fold_h4": fold_h4, "ge": ge,
          "g_ripple": g_ripple if ge else 0, "pad_carry": tuple(pad_carry[:3])}
    return tag.to_bytes(16, "little"), br


def steer_carry_out(key, lens, k, rng, head=b""):
    """A message in pieces (as steer_pieces) whose joined radix-2^26 value is 2^131 - k (k = 1..5)
    before reduction, the one input class on which f26_to32 carries out of limb 4.  The last piece's
    partial is a residue T_last that the device holds as T_last + p = 2^130 + (T_last - 5), h4 = 4
    (any 5 <= T_last < 2^96), and the pieces before it end at G with G * r^m = 10 - k - T_last, which
    f26_mul returns as 2^130 - (T_last - 5) - k.  Returns (message, pieces)."""
    assert 1 <= k <= 5 and len(lens) >= 2 and lens[-1] >= 32
    T_last = rng.randrange(5, 1 << 90)
    last = steer_from(key, 0, lens[-1], T_last, rng)
    assert limbs_value(device_state(last, key)) == T_last + P
    m = (lens[-1] + 15) // 16
    G = (10 - k - T_last) * pow(key_r(key), -m, P) % P
    front = steer_pieces(key, lens[:-1], [PARTIALS[i % len(PARTIALS)] for i in range(len(lens) - 1)], G, rng, head)
    msg = front + last
    assert accumulate(msg, key) == 10 - k
    pieces, o = [], 0
    for n in lens:
        pieces.append(msg[o:o + n])
        o += n
    return msg, pieces
