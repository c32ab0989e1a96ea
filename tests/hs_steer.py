"""Steered CURVE handshake commands: the batched handshake kernels at their Poly1305 and X25519 edges.

poly_steer.py and x25519_steer.py put the rare branches of poly_block / poly_finish and of
fe_to_words under cz_kernels.hip and k_x25519.  The handshake translation unit instantiates the same
inline arithmetic again -- xs_fixed<4> / xs_fixed<8> unrolled over registers, xs_mem with its
run-time length and partial last chunk, k_x25519_jobs with its own loads, flags and stores -- and
everything the peer sends is attacker-chosen.  This module builds whole handshakes, through the
public commands only, in which one box's Poly1305 accumulator ends at a poly_steer target or one key
agreement ends at an x25519_steer target; tests/hs_model.py (added functions included) is the
reference for every byte.  Helper of test_hs_steer.py (CPU) and test_gpu_hs_edges.py; no GPU.

Poly1305: the key of a box is box_keystream(k, n24, 32) and the MAC runs over the ciphertext, so a
box is steerable where the sender or the test is free to choose two ciphertext blocks:
  HELLO box (opened by k_acc_welcome)         the whole 64-byte body: only the tag is checked
  cookie (sealed by k_acc_welcome, opened     plaintext C' + s' with s' injected: the last two chunks
          by k_acc_initiate)
  INITIATE box (opened by k_acc_initiate,     the value of the trailing Identity property
          sealed by k_con_initiate)
  READY box (sealed by k_acc_ready,           the acceptor's own identity; as the client sees it, any
          opened by k_con_ready)              metadata value
  WELCOME box (opened by k_con_welcome)       the 96 cookie bytes, opaque to the client
Three boxes are not steerable without grinding through keys or nonces, and nothing here grinds: the
vouch (its plaintext C' + S is fixed by the check that follows the open), the WELCOME seal (the
cookie in it depends on the only free block before it) and the connector's HELLO seal (its plaintext
is 64 zero bytes).

X25519: x25519_steer.steered_cases(k) solves the point u with X25519(k, u) = t.  Whoever sends such
a point -- or a non-canonical or low-order one -- holds no secret for it; the key both sides end at is
HSalsa20(0^16, X25519(k, u)) by the big-integer ladder x25519_ref, and the peer's commands are sealed
under it directly (hs_model.*_under).  The model's own side computes the same agreement through the
oracle and refuses the command when the two differ, so every lane built here is one on which
x25519_ref, the oracle and the model agree.

Everything is deterministic from the names and indices given, and every builder raises when a case
cannot be built: a case list never shrinks silently.
"""
import functools
import random
import struct

import hs_model as M
import poly_steer as ps
import x25519_steer as xs
from cz_testlib import or_beforenm, or_hsalsa20
from test_gpu_x25519_edges import LOW_ORDER
from test_hs_model import CLIENT_PUB, CLIENT_SEC, SERVER_PUB, SERVER_SEC

ZMQ_DEALER, ZMQ_ROUTER = 5, 6
P255 = xs.P
M32 = ps.M32


def _b(v):
    return v.to_bytes(32, "little")


def xor(a, b):
    return bytes(x ^ y for x, y in zip(a, b))


def be64(n):
    return struct.pack(">Q", n)


def hsalsa(shared):
    """NaCl's beforenm on a shared secret"""
    return or_hsalsa20(bytes(16), shared)


# ---- Poly1305 ---------------------------------------------------------------------------------
TARGET = dict(ps.TARGETS)
HM = ("hm-ripple-0", "hm-ripple-3")
ALL_POLY = [n for n, _ in ps.TARGETS] + list(HM)
# what one acceptor or connector instance per case can afford: the two sides of the freeze, the three
# h4 boundaries, an all-ones ripple, a fold, the pad additions, the h + m chain
PER_INSTANCE = ["freeze+0", "freeze+4", "freeze+5", "freeze-p-1", "freeze-p-5", "h4-1*2^128+0", "h4-2*2^128-1",
                "h4-3*2^128+1", "ripple-2^128-1", "fold-2^64+0", "pad-tag-zero", "pad-tag-ones", "pad-ripple-from-0",
                "hm-ripple-0"]
assert set(PER_INSTANCE) <= set(ALL_POLY)


def reaches(name, ct, key, seen=None):
    """Does the ciphertext `ct` take, on the restated device arithmetic (test_poly_radix32.poly_block,
    poly_steer.device_finish), the branch its target is named for?  seen: a dict of sets that
    collects what the rare paths did, for a per-path census."""
    s = ps.key_s(key)
    h = ps.device_state(ct, key)
    tag, br = ps.device_finish(h, s)
    if tag != ps.poly1305(ct, key):
        raise AssertionError(f"{name}: the restated device arithmetic and the big-integer Poly1305 differ")
    if seen is not None:
        seen.setdefault("ge", set()).add(br["ge"])
        seen.setdefault("h4", set()).add(h[4])
        seen.setdefault("g_ripple", set()).add(br["g_ripple"])
        seen.setdefault("pad_carry", set()).add(br["pad_carry"])
        if br["fold"]:
            seen.setdefault("fold_ripple", set()).add(br["fold_ripple"])
    v = ps.limbs_value(h)
    if name in HM:
        x = int(name.rsplit("-", 1)[1])
        cut = len(ct) // 16 * 16 - 16
        last = int.from_bytes(ct[cut:cut + 16], "little")
        return ps.device_state(ct[:cut], key) == (M32 - x, M32, M32, M32, 0) and last == (x + 1) | (ps.M128 >> 32 << 32)
    raw = TARGET[name](s)
    T = raw % ps.P
    if v not in (T, T + ps.P):          # the device holds the residue partially reduced
        return False
    if name.startswith("freeze+"):      # at the conditional subtraction: p + d is subtracted or folded, d is neither
        return br["ge"] == (ps.P <= v < 1 << 130) and br["fold"] == v >> 130
    if name.startswith("freeze-p-"):    # the largest values that are not subtracted
        return v == T and not br["ge"] and not br["fold"]
    if name.startswith("h4-"):
        return v == raw and h[4] == raw >> 128
    if name.startswith("ripple-"):
        return v == raw if raw < ps.P and raw >= 1 << 97 else True
    if name.startswith("fold-"):        # held as 2^130 + (T - 5): the fold's carry crosses k / 32 limbs
        k = int(name[7:].split("+")[0])
        return br["fold"] == 1 and br["fold_ripple"] == k // 32
    if name == "pad-tag-zero":
        return tag == bytes(16)
    if name == "pad-tag-ones":
        return tag == b"\xff" * 16
    if name.startswith("pad-ripple-from-"):
        j = int(name[-1])
        return br["pad_carry"] == tuple(int(i >= j) for i in range(3))
    raise KeyError(name)


def steer_box(k, n24, nbytes, name, rng, head_plain=b""):
    """A box of nbytes under key k and nonce n24 whose plaintext starts with head_plain and whose
    Poly1305 takes the branch `name`: (plaintext, tag + ciphertext, the one-time key)"""
    ks = ps.box_keystream(k, n24, 32 + nbytes)
    key = ks[:32]
    head = xor(head_plain, ks[32:])
    if name in HM:
        ct = ps.hm_ripple(key, nbytes, int(name.rsplit("-", 1)[1]), rng, head)
    else:
        ct = ps.steer(key, nbytes, TARGET[name](ps.key_s(key)), rng, head, accept=lambda m: reaches(name, m, key))
    if not reaches(name, ct, key) or len(ct) != nbytes or not ct.startswith(head):
        raise RuntimeError(f"{name}: the steered box of {nbytes} bytes misses its branch")
    return xor(ct, ks[32:]), ps.poly1305(ct, key) + ct, key


def steer_cookie_hm(name, cp, rng):
    """hm-ripple on the cookie: C' fills the first two chunks, so nothing before the solved chunk can be
    redrawn but the cookie key and nonce themselves.  (entropy 64, s')"""
    x = int(name.rsplit("-", 1)[1])
    want = (1 << 128) - 1 - x
    last = ((x + 1) | (ps.M128 >> 32 << 32)).to_bytes(16, "little")
    for _ in range(ps.MAX_DRAWS):
        entropy = rng.randbytes(64)
        ks = ps.box_keystream(entropy[16:48], b"COOKIE--" + entropy[:16], 96)
        key = ks[:32]
        head = xor(cp, ks[32:])
        r = ps.key_r(key)
        if r == 0:
            continue
        v = (want * pow(r, -1, ps.P) - ps.accumulate(head, key)) % ps.P
        if v >> 128 != 1:
            continue
        ct = head + (v & ps.M128).to_bytes(16, "little") + last
        if reaches(name, ct, key):
            return entropy, xor(ct, ks[32:])[32:], ct, key
    raise RuntimeError(f"{name}: no cookie key in {ps.MAX_DRAWS} draws")


# ---- X25519 -----------------------------------------------------------------------------------
# the scalars of the six jobs: the long-term s and c, and one injected short-term secret per side
EPH_S = random.Random("hs_steer s'").randbytes(32)
EPH_C = random.Random("hs_steer c'").randbytes(32)
JOB_SCALAR = {"acc k1": SERVER_SEC, "acc cnPrecom": EPH_S, "acc k3": EPH_S,
              "con kH": EPH_C, "con cnPrecom": EPH_C, "con kV": CLIENT_SEC}
EXTREME_SCALARS = {"zero": bytes(32), "ones": b"\xff" * 32, "clamped-bits-only": bytes(31) + b"\x40"}


@functools.lru_cache(maxsize=None)
def points(scalar):
    """[(kind, name, u)]: the points one key-agreement job is given under `scalar` -- the 33 steered
    ones of x25519_steer.CLASSES, the non-canonical ones (p .. p + 18, 2^255 - 1, a valid key with bit
    255 set) and the low-order ones"""
    out = [("steered", f"{cls} t={t:#x}", u) for cls, t, u in xs.steered_cases(scalar)]
    if len(out) != 33:
        raise RuntimeError(f"{len(out)} steered cases, not 33")
    out += [("noncanonical", f"p+{d}", _b(P255 + d)) for d in range(19)]
    out.append(("noncanonical", "2^255-1", _b((1 << 255) - 1)))
    valid = int.from_bytes(M.public_key(random.Random("hs_steer valid").randbytes(32)), "little")
    out.append(("noncanonical", "valid-key|2^255", _b(valid | 1 << 255)))
    out += [("low-order", f"{v:#x}", _b(v)) for v in LOW_ORDER]
    return out


def agreed(scalar, u):
    """the key beforenm(u, scalar) must give: by the big-integer ladder, never by the code under test"""
    return hsalsa(xs.x25519_ref(scalar, u))


# ---- the acceptor's peers ---------------------------------------------------------------------
HELLO_TAG, COOKIE_TAG, INITIATE_TAG = 120, 25, 113      # where the three tags the acceptor checks lie
WELCOME_TAG, READY_TAG = 24, 14                         # and the connector's two
INIT_LENS = [29, 48, 49, 60, 61, 62, 63, 100, 221]      # identity lengths of a steered INITIATE (box of 163 + n)
SEAL_LENS = [60, 61, 62, 221, 29]                       # identity lengths of a steered seal
READY_LENS = [32, 33, 47, 48, 95, 96, 97, 111, 256]     # plaintext lengths of a steered READY as the client sees it
assert {(32 + 163 + n) % 64 for n in INIT_LENS[3:6]} == {63, 0, 1}          # a Salsa20 block edge and +-1
assert {(163 + n) % 16 for n in INIT_LENS} >= {0, 1, 15} and max(INIT_LENS) == 221
assert {(35 + n) % 16 for n in SEAL_LENS} >= {0, 1, 15} and (32 + 35 + 61) % 64 == 0
assert {n % 16 for n in READY_LENS} >= {0, 1, 15} and READY_LENS[0] == 32 and {(32 + n) % 64 for n in READY_LENS} >= {63, 0, 1}


def acc_lane(name, seed, cli_eph=None, k1=None, precom=None, cpub=None, k3=None, seph=None, hello=None, cookie=None,
             initiate=None, ready=None, x=None):
    """One connection as a CurveAcceptor (long-term key SERVER_SEC, ROUTER) sees it from a DEALER peer.
    cli_eph / cpub: the C' / C the peer sends instead of an honest one, with k1, precom, k3 the keys the
    agreements on them end at.  seph: the injected s'.  hello / cookie: a Poly1305 target for that box;
    initiate / ready: (target, identity length) for the INITIATE box / the acceptor's READY seal.
    x: {job: (kind, point name)} for the census.  Raises when the model refuses any of it."""
    rng = random.Random(f"acc {name} {seed}")
    ceph, csec, vnonce, entropy = rng.randbytes(32), rng.randbytes(32), rng.randbytes(16), rng.randbytes(64)
    seph = rng.randbytes(32) if seph is None else seph
    cp = M.public_key(ceph) if cli_eph is None else cli_eph
    k1 = or_beforenm(cp, SERVER_SEC) if k1 is None else k1
    poly, hbox = {}, None
    if hello:
        _, hbox, key = steer_box(k1, b"CurveZMQHELLO---" + be64(1), 64, hello, rng)
        poly["hello"] = (hello, hbox[16:], key)
    if cookie:
        if cookie in HM:
            entropy, seph, ct, key = steer_cookie_hm(cookie, cp, rng)
        else:
            plain, cbox, key = steer_box(entropy[16:48], b"COOKIE--" + entropy[:16], 64, cookie, rng, head_plain=cp)
            seph, ct = plain[32:], cbox[16:]
        poly["cookie"] = (cookie, ct, key)
    hello_cmd = M.hello_under(k1, cp, box=hbox)
    got = M.server_welcome(hello_cmd, SERVER_SEC, seph, entropy)
    if got is None or got[1] is None:
        raise RuntimeError(f"{name}: the model server refuses the HELLO")
    welcome, state = got
    opened = M._open(welcome[24:], b"WELCOME-" + welcome[8:24], k1)
    if opened is None or opened[:32] != M.public_key(seph):
        raise RuntimeError(f"{name}: the WELCOME does not open under k1")
    sp, cookie96 = opened[:32], opened[32:]
    if cookie and cookie96[32:] != poly["cookie"][1]:
        raise RuntimeError(f"{name}: the model's cookie is not the steered one")
    precom = or_beforenm(cp, seph) if precom is None else precom
    if precom != state["precom"]:
        raise RuntimeError(f"{name}: cnPrecom differs from the model's")
    C = M.public_key(csec) if cpub is None else cpub
    k3 = or_beforenm(sp, csec) if k3 is None else k3
    head = C + vnonce + M.vouch_under(k3, vnonce, cp, SERVER_PUB)
    ibox, cident, sident = None, b"", b""
    if initiate:
        target, n = initiate
        mhead = M.metadata(ZMQ_DEALER, bytes(n))[:35]
        plain, ibox, key = steer_box(precom, b"CurveZMQINITIATE" + be64(2), 163 + n, target, rng, head_plain=head + mhead)
        cident = plain[163:]
        poly["initiate"] = (target, ibox[16:], key)
    plain = head + M.metadata(ZMQ_DEALER, cident)
    init_cmd = M.initiate_under(cookie96, precom, plain)
    if ibox is not None and init_cmd[113:] != ibox:
        raise RuntimeError(f"{name}: the model's INITIATE box is not the steered one")
    if ready:
        target, n = ready
        mhead = M.metadata(ZMQ_ROUTER, bytes(n))[:35]
        rplain, rbox, key = steer_box(precom, b"CurveZMQREADY---" + be64(1), 35 + n, target, rng, head_plain=mhead)
        sident = rplain[35:]
        poly["ready"] = (target, rbox[16:], key)
    got = M.server_ready(init_cmd, state, socket_type=ZMQ_ROUTER, identity=sident)
    if isinstance(got, str):
        raise RuntimeError(f"{name}: the model server refuses the INITIATE: {got}")
    ready_cmd, facts = got
    if ready and ready_cmd[14:] != rbox:
        raise RuntimeError(f"{name}: the model's READY box is not the steered one")
    assert facts["client_key"] == C and facts["metadata"] == M.metadata(ZMQ_DEALER, cident)
    return {"side": "acc", "name": name, "seph": seph, "entropy": entropy, "hello": hello_cmd, "welcome": welcome,
            "state": state, "initiate": init_cmd, "ready": ready_cmd, "precom": precom, "client_key": C,
            "peer_identity": cident, "sident": sident, "flip": None, "poly": poly, "x": x or {}, "cp": cp,
            "k1": k1, "k3": k3, "sp": sp}


def con_lane(name, seed, spub=None, kh=None, srv_eph=None, precom=None, ceph=None, welcome=None, initiate=None,
             ready=None, x=None):
    """One connection as a CurveConnector (CLIENT_PUB / CLIENT_SEC, DEALER) sees it.  spub / srv_eph: the S
    given to hello() / the S' in the WELCOME box instead of honest ones, with kh and precom the keys the
    agreements on them end at.  ceph: the injected c'.  welcome: a Poly1305 target for the WELCOME box
    (through its cookie bytes); initiate: (target, identity length) for the connector's INITIATE seal;
    ready: (target, plaintext length) for the READY box (through a metadata value)."""
    rng = random.Random(f"con {name} {seed}")
    ssec, seph, vnonce, entropy = rng.randbytes(32), rng.randbytes(32), rng.randbytes(16), rng.randbytes(64)
    ceph = rng.randbytes(32) if ceph is None else ceph
    S = M.public_key(ssec) if spub is None else spub
    cp = M.public_key(ceph)
    hello_cmd = M.client_hello(S, ceph)
    kh = or_beforenm(S, ceph) if kh is None else kh
    sp = M.public_key(seph) if srv_eph is None else srv_eph
    wnonce = entropy[48:64]
    poly = {}
    if welcome:
        plain, wbox, key = steer_box(kh, b"WELCOME-" + wnonce, 128, welcome, rng, head_plain=sp)
        cookie96 = plain[32:]
        poly["welcome"] = (welcome, wbox[16:], key)
    else:
        cookie96 = entropy[:16] + M._seal(cp + seph, b"COOKIE--" + entropy[:16], entropy[16:48])
    welcome_cmd = M.welcome_under(kh, sp, cookie96, wnonce)
    if welcome and welcome_cmd[24:] != wbox:
        raise RuntimeError(f"{name}: the model's WELCOME box is not the steered one")
    if M.client_open_welcome(welcome_cmd, S, ceph) != (sp, cookie96):
        raise RuntimeError(f"{name}: the model client refuses the WELCOME")
    precom = or_beforenm(sp, ceph) if precom is None else precom
    kv = or_beforenm(sp, CLIENT_SEC)
    cident, ibox = b"", None
    if initiate:
        target, n = initiate
        head = CLIENT_PUB + vnonce + M.vouch_under(kv, vnonce, cp, S) + M.metadata(ZMQ_DEALER, bytes(n))[:35]
        plain, ibox, key = steer_box(precom, b"CurveZMQINITIATE" + be64(2), 163 + n, target, rng, head_plain=head)
        cident = plain[163:]
        poly["initiate"] = (target, ibox[16:], key)
    init_cmd = M.client_initiate(welcome_cmd, CLIENT_PUB, CLIENT_SEC, S, ceph, vnonce, socket_type=ZMQ_DEALER,
                                 identity=cident)
    if ibox is not None and init_cmd[113:] != ibox:
        raise RuntimeError(f"{name}: the model's INITIATE box is not the steered one")
    if init_cmd[9:105] != cookie96 or M._open(init_cmd[113:], b"CurveZMQINITIATE" + be64(2), precom) is None:
        raise RuntimeError(f"{name}: the model's INITIATE does not open under cnPrecom")
    value, rbox = b"", None
    typed = M.prop(b"Socket-Type", b"ROUTER")
    if ready:
        target, n = ready
        mhead = (typed if n >= 48 else b"") + M.prop(b"X", bytes(n))[:6]
        n_value = n - len(mhead)
        mhead = mhead[:-4] + struct.pack(">I", n_value)
        rplain, rbox, key = steer_box(precom, b"CurveZMQREADY---" + be64(1), n, target, rng, head_plain=mhead)
        value = rplain[len(mhead):]
        meta = rplain
        assert meta == mhead + value and meta.endswith(M.prop(b"X", value))
        poly["ready"] = (target, rbox[16:], key)
    else:
        meta = typed + M.prop(b"X", value)
    ready_cmd = M.ready_under(precom, meta)
    if rbox is not None and ready_cmd[14:] != rbox:
        raise RuntimeError(f"{name}: the model's READY box is not the steered one")
    if M.client_open_ready(ready_cmd, sp, ceph) != meta:
        raise RuntimeError(f"{name}: the model client refuses the READY")
    return {"side": "con", "name": name, "ceph": ceph, "vnonce": vnonce, "spub": S, "hello": hello_cmd,
            "welcome": welcome_cmd, "initiate": init_cmd, "ready": ready_cmd, "precom": precom, "cident": cident,
            "peer_type": b"ROUTER" if meta.startswith(typed) else None, "peer_x": value, "flip": None, "poly": poly,
            "x": x or {}, "sp": sp, "kh": kh, "kv": kv}


# ---- refusals ---------------------------------------------------------------------------------
FLIP_AT = {"hello": ("hello", HELLO_TAG), "cookie": ("initiate", COOKIE_TAG), "initiate": ("initiate", INITIATE_TAG),
           "welcome": ("welcome", WELCOME_TAG), "ready": ("ready", READY_TAG)}


def flipped(lane, box, word, bit):
    """the lane again with one bit of `box`'s tag flipped in the command that carries it"""
    cmd, base = FLIP_AT[box]
    b = bytearray(lane[cmd])
    b[base + 4 * word + bit // 8] ^= 1 << (bit % 8)
    out = dict(lane)
    out[cmd] = bytes(b)
    out["flip"] = box
    out["name"] = f"{lane['name']} flip {box} word {word} bit {bit}"
    return out


def flips(lane, box, i):
    """One flipped copy; for the all-zero and all-ones tags one per tag word, since a compare that
    skips a word accepts one of them"""
    if lane["poly"][box][0] in ("pad-tag-zero", "pad-tag-ones"):
        return [flipped(lane, box, w, (11 * w + 5 * i) % 32) for w in range(4)]
    return [flipped(lane, box, i % 4, (7 * i) % 32)]


def model_refuses(lane):
    """Does hs_model refuse a flipped lane's command, at the check the flip aims at?"""
    box = lane["flip"]
    if box == "hello":
        return M.server_welcome(lane["hello"], SERVER_SEC, lane["seph"], lane["entropy"]) == (M.ERROR_EMPTY, None)
    if box in ("cookie", "initiate"):
        return M.server_ready(lane["initiate"], lane["state"], socket_type=ZMQ_ROUTER,
                              identity=lane["sident"]) == "cryptographic"
    if box == "welcome":
        w = lane["welcome"]
        return M._open(w[24:], b"WELCOME-" + w[8:24], lane["kh"]) is None
    if box == "ready":
        r = lane["ready"]
        return M._open(r[14:], b"CurveZMQREADY---" + r[6:14], lane["precom"]) is None
    raise KeyError(box)


# ---- the case lists ---------------------------------------------------------------------------
def _with_flips(lanes, box):
    out = []
    for i, lane in enumerate(lanes):
        out.append(lane)
        out += flips(lane, box, i)
    return out


@functools.lru_cache(maxsize=None)
def acc_hello_lanes():
    """HELLO boxes steered to every target; every second one on a C' steered for the server's secret"""
    pts = [p for p in points(SERVER_SEC) if p[0] == "steered"]
    out = []
    for i, name in enumerate(ALL_POLY):
        kw = {}
        if i % 2:
            kind, pname, u = pts[i % len(pts)]
            kw = {"cli_eph": u, "k1": agreed(SERVER_SEC, u), "x": {"acc k1": (kind, pname, SERVER_SEC, u)}}
        out.append(acc_lane(f"hello {name}", i, hello=name, **kw))
    return _with_flips(out, "hello")


@functools.lru_cache(maxsize=None)
def acc_cookie_lanes():
    return _with_flips([acc_lane(f"cookie {name}", i, cookie=name) for i, name in enumerate(ALL_POLY)], "cookie")


@functools.lru_cache(maxsize=None)
def acc_initiate_lanes(rot):
    """INITIATE boxes steered to every target, target i at identity length INIT_LENS[(i + 3 * rot) % 9]:
    rot = 0, 1, 2 put every target at three lengths and every length under 16 targets or more"""
    out = []
    for i, name in enumerate(ALL_POLY):
        n = INIT_LENS[(i + 3 * rot) % len(INIT_LENS)]
        if name in HM and n < 48:       # the h + m chain needs a free chunk before the solved one
            n = 221
        out.append(acc_lane(f"initiate {name} rot {rot}", i, initiate=(name, n)))
    return _with_flips(out, "initiate")


@functools.lru_cache(maxsize=None)
def acc_ready_lanes():
    """one per acceptor instance: the READY it seals is steered through its own identity"""
    return [acc_lane(f"ready {name}", i, ready=(name, SEAL_LENS[i % len(SEAL_LENS)])) for i, name in enumerate(PER_INSTANCE)]


ACC_JOBS = ("acc k1", "acc cnPrecom", "acc k3")
CON_JOBS = ("con kH", "con cnPrecom", "con kV")


@functools.lru_cache(maxsize=None)
def acc_x_lanes(job):
    k = JOB_SCALAR[job]
    out = []
    for i, (kind, pname, u) in enumerate(points(k)):
        x = {job: (kind, pname, k, u)}
        key = agreed(k, u)
        if job == "acc k1":
            kw = {"cli_eph": u, "k1": key}
        elif job == "acc cnPrecom":
            kw = {"cli_eph": u, "precom": key, "seph": k}
        else:
            kw = {"cpub": u, "k3": key, "seph": k}
        out.append(acc_lane(f"{job} {kind} {pname}", i, x=x, **kw))
    return out


@functools.lru_cache(maxsize=None)
def acc_base_lanes():
    """S' = s' . 9 at the extreme scalars (the base-point result cannot be steered)"""
    return [acc_lane(f"acc base {n}", i, seph=k, x={"acc base": ("extreme-scalar", n, k, M.BASE)})
            for i, (n, k) in enumerate(EXTREME_SCALARS.items())]


@functools.lru_cache(maxsize=None)
def con_welcome_lanes():
    return _with_flips([con_lane(f"welcome {name}", i, welcome=name) for i, name in enumerate(ALL_POLY)], "welcome")


@functools.lru_cache(maxsize=None)
def con_initiate_lanes():
    """one per connector instance: the INITIATE it seals is steered through its own identity"""
    return [con_lane(f"initiate {name}", i, initiate=(name, SEAL_LENS[i % len(SEAL_LENS)]))
            for i, name in enumerate(PER_INSTANCE)]


@functools.lru_cache(maxsize=None)
def con_ready_lanes(rot):
    """READY boxes steered to every target, target i at plaintext length READY_LENS[(i + 3 * rot) % 9]; the
    h + m chain needs two chunks before its last one, so it goes to the lengths from 95 bytes on"""
    out = []
    for i, name in enumerate(ALL_POLY):
        n = READY_LENS[(i + 3 * rot) % len(READY_LENS)]
        if name in HM:
            n = READY_LENS[4 + (i + rot) % 5]
        out.append(con_lane(f"ready {name} rot {rot}", i, ready=(name, n)))
    return _with_flips(out, "ready")


@functools.lru_cache(maxsize=None)
def con_x_lanes(job):
    k = JOB_SCALAR[job]
    out = []
    for i, (kind, pname, u) in enumerate(points(k)):
        x = {job: (kind, pname, k, u)}
        key = agreed(k, u)
        if job == "con kH":
            kw = {"spub": u, "kh": key, "ceph": k}
        elif job == "con cnPrecom":
            kw = {"srv_eph": u, "precom": key, "ceph": k}
        else:
            kw = {"srv_eph": u}
        lane = con_lane(f"{job} {kind} {pname}", i, x=x, **kw)
        if job == "con kV" and lane["kv"] != key:
            raise RuntimeError(f"{lane['name']}: the model's vouch key is not the agreed one")
        out.append(lane)
    return out


@functools.lru_cache(maxsize=None)
def con_base_lanes():
    return [con_lane(f"con base {n}", i, ceph=k, x={"con base": ("extreme-scalar", n, k, M.BASE)})
            for i, (n, k) in enumerate(EXTREME_SCALARS.items())]


ROTS = (0, 1, 2)


def all_lanes():
    """every lane of every list above, as the two test modules run them"""
    out = acc_hello_lanes() + acc_cookie_lanes() + acc_ready_lanes() + acc_base_lanes()
    out += con_welcome_lanes() + con_initiate_lanes() + con_base_lanes()
    for rot in ROTS:
        out += acc_initiate_lanes(rot) + con_ready_lanes(rot)
    for job in ACC_JOBS:
        out += acc_x_lanes(job)
    for job in CON_JOBS:
        out += con_x_lanes(job)
    return out


# the kernel paths of the census: (row, side, the box or job a lane must carry)
PATHS = [
    ("xs_fixed<4,true> in k_acc_welcome: HELLO box", "acc", "hello"),
    ("xs_fixed<4,false> in k_acc_welcome, xs_fixed<4,true> in k_acc_initiate: cookie", "acc", "cookie"),
    ("xs_mem<true> in k_acc_initiate: INITIATE box", "acc", "initiate"),
    ("xs_mem<false> in k_acc_ready: READY seal", "acc", "ready"),
    ("xs_fixed<8,true> in k_con_welcome: WELCOME box", "con", "welcome"),
    ("xs_mem<false> in k_con_initiate: INITIATE seal", "con", "initiate"),
    ("xs_mem<true> in k_con_ready: READY box", "con", "ready"),
    ("k_x25519_jobs, acceptor stage 1: k1 = beforenm(C', s)", "acc", "acc k1"),
    ("k_x25519_jobs, acceptor stage 1: cnPrecom = beforenm(C', s')", "acc", "acc cnPrecom"),
    ("k_x25519_jobs, acceptor stage 2: k3 = beforenm(C, s')", "acc", "acc k3"),
    ("k_x25519_jobs, connector stage 1: kH = beforenm(S, c')", "con", "con kH"),
    ("k_x25519_jobs, connector stage 2: cnPrecom = beforenm(S', c')", "con", "con cnPrecom"),
    ("k_x25519_jobs, connector stage 2: kV = beforenm(S', c)", "con", "con kV"),
    ("k_x25519_jobs, base point: S' = s'.9", "acc", "acc base"),
    ("k_x25519_jobs, base point: C' = c'.9", "con", "con base"),
]


def census():
    """[(row, steered cases run, of them Poly1305 targets, of them X25519 classes)], counted from the lanes
    the tests run; the refused copies (one tag bit flipped) are not counted"""
    lanes = [x for x in all_lanes() if x["flip"] is None]
    rows = []
    for row, side, what in PATHS:
        mine = [x for x in lanes if x["side"] == side and (what in x["poly"] or what in x["x"])]
        rows.append((row, len(mine), sum(1 for x in mine if x["poly"]),
                     sum(1 for x in mine if any(v[0] == "steered" for v in x["x"].values()))))
    return rows


if __name__ == "__main__":
    print("| kernel path | steered cases | Poly1305 targets | X25519 classes |\n|---|---|---|---|")
    for r in census():
        print("| " + " | ".join(str(c) for c in r) + " |")
