"""A model of both sides of the CURVE handshake (RFC 26; CurveClientMechanism.java:246-385,
CurveServerMechanism.java:254-507) built only on the CPU oracle helpers of cz_testlib, with every
secret and every random draw injected.  Test infrastructure: tests/test_hs_model.py anchors it to
the recorded libzmq sessions, and the GPU tests of the batched acceptor use it as their yardstick.

Commands are ZMTP command bodies.  Boxes: or_box(m, n24, pk, sk) returns 16 zero bytes, the tag and
the ciphertext, so [16:] is what travels."""
import struct

from cz_testlib import or_beforenm, or_box, or_box_afternm, or_box_open_afternm, or_x25519

BASE = (9).to_bytes(32, "little")
SOCKET_NAMES = ["PAIR", "PUB", "SUB", "REQ", "REP", "DEALER", "ROUTER", "PULL", "PUSH", "XPUB", "XSUB", "STREAM",
                "SERVER", "CLIENT", "RADIO", "DISH", "CHANNEL", "PEER", "RAW", "SCATTER", "GATHER"]
ERROR_EMPTY = b"\x05ERROR\x00"


class ModelError(ValueError):
    pass


def public_key(secret):
    return or_x25519(secret, BASE)


def prop(name, value):
    return bytes([len(name)]) + name + struct.pack(">I", len(value)) + value


def metadata(socket_type, identity=b""):
    """Mechanism.addProperty: Socket-Type and, for REQ / DEALER / ROUTER, Identity"""
    m = prop(b"Socket-Type", SOCKET_NAMES[socket_type].encode())
    if socket_type in (3, 5, 6):
        m += prop(b"Identity", bytes(identity))
    return m


def _seal(m, n24, k):
    rc, c = or_box_afternm(bytes(32) + bytes(m), bytes(n24), k)
    assert rc == 0
    return c[16:]


def _open(boxed, n24, k):
    """tag + ciphertext -> plaintext, or None"""
    rc, m = or_box_open_afternm(bytes(16) + bytes(boxed), bytes(n24), k)
    return m[32:] if rc == 0 else None


# ---- client ---------------------------------------------------------------------------------
def client_hello(server_key, eph_secret, nonce=1):
    """produceHello: Box [64 * %x0](C'->S)"""
    n8 = struct.pack(">Q", nonce)
    box = or_box(bytes(64), b"CurveZMQHELLO---" + n8, server_key, eph_secret)[16:]
    return b"\x05HELLO\x01\x00" + bytes(72) + public_key(eph_secret) + n8 + box


def client_open_welcome(welcome, server_key, eph_secret):
    """processWelcome: (S', cookie 96) or None"""
    if len(welcome) != 168 or welcome[:8] != b"\x07WELCOME":
        return None
    p = _open(welcome[24:], b"WELCOME-" + welcome[8:24], or_beforenm(server_key, eph_secret))
    return None if p is None else (p[:32], p[32:128])


def client_initiate(welcome, public, secret, server_key, eph_secret, vouch_nonce, socket_type=0, identity=b"",
                    nonce=2, meta=None, vouch_eph_public=None, vouch_server_key=None, vouch_flip=None):
    """produceInitiate from a WELCOME: cookie + nonce + Box [C + vouch + metadata](C'->S'), vouch =
    Box [C',S](C->S').  meta / vouch_* override what an honest client sends (failure cases); vouch_flip
    = index of a vouch byte whose low bit is flipped before the INITIATE box is sealed."""
    got = client_open_welcome(welcome, server_key, eph_secret)
    if got is None:
        raise ModelError("WELCOME does not open")
    srv_eph, cookie = got
    if meta is None:
        meta = metadata(socket_type, identity)
        if len(meta) > 256:  # "Assume here that metadata is limited to 256 bytes"
            raise ModelError(f"INITIATE metadata of {len(meta)} bytes exceeds 256")
    vp = (vouch_eph_public if vouch_eph_public is not None else public_key(eph_secret)) + \
        (vouch_server_key if vouch_server_key is not None else server_key)
    vouch = or_box(vp, b"VOUCH---" + bytes(vouch_nonce), srv_eph, secret)[16:]
    if vouch_flip is not None:
        vouch = vouch[:vouch_flip] + bytes([vouch[vouch_flip] ^ 1]) + vouch[vouch_flip + 1:]
    n8 = struct.pack(">Q", nonce)
    box = or_box(bytes(public) + bytes(vouch_nonce) + vouch + meta, b"CurveZMQINITIATE" + n8, srv_eph, eph_secret)[16:]
    return b"\x08INITIATE" + cookie + n8 + box


def client_open_ready(ready, srv_eph, eph_secret):
    """processReady: the server's metadata, or None"""
    if len(ready) < 30 or ready[:6] != b"\x05READY":
        return None
    return _open(ready[14:], b"CurveZMQREADY---" + ready[6:14], or_beforenm(srv_eph, eph_secret))


# ---- server ---------------------------------------------------------------------------------
def server_welcome(hello, server_secret, eph_secret, entropy):
    """processHello + produceWelcome with entropy = cookie nonce 16, cookie key 32, WELCOME nonce 16.
    Returns (WELCOME, state) or (ERROR, None) when the HELLO box does not open; None for a malformed
    HELLO."""
    if len(hello) != 200 or hello[:8] != b"\x05HELLO\x01\x00":
        return None
    cli_eph = hello[80:112]
    k1 = or_beforenm(cli_eph, server_secret)
    if _open(hello[120:200], b"CurveZMQHELLO---" + hello[112:120], k1) is None:
        return ERROR_EMPTY, None
    cnonce, ckey, wnonce = entropy[:16], entropy[16:48], entropy[48:64]
    cookie = _seal(cli_eph + bytes(eph_secret), b"COOKIE--" + cnonce, ckey)
    wbox = _seal(public_key(eph_secret) + cnonce + cookie, b"WELCOME-" + wnonce, k1)
    state = {"cli_eph": cli_eph, "eph_secret": bytes(eph_secret), "cookie_key": ckey,
             "precom": or_beforenm(cli_eph, eph_secret)}
    return b"\x07WELCOME" + wnonce + wbox, state


def server_ready(initiate, state, socket_type=0, identity=b"", nonce=1):
    """processInitiate + produceReady.  Returns (READY, facts) with facts = client_key, metadata and
    precom, or a string naming the first check that failed."""
    if initiate[:9] != b"\x08INITIATE":
        return "unexpected"
    if len(initiate) < 257 or len(initiate) - 113 > 144 + 256:
        return "malformed"
    kp = _open(initiate[25:105], b"COOKIE--" + initiate[9:25], state["cookie_key"])
    if kp is None or kp[:32] != state["cli_eph"] or kp[32:] != state["eph_secret"]:
        return "cryptographic"
    ip = _open(initiate[113:], b"CurveZMQINITIATE" + initiate[105:113], state["precom"])
    if ip is None:
        return "cryptographic"
    client_key, vnonce, vouch, meta = ip[:32], ip[32:48], ip[48:128], ip[128:]
    vp = _open(vouch, b"VOUCH---" + vnonce, or_beforenm(client_key, state["eph_secret"]))
    if vp is None:
        return "cryptographic"
    if vp[:32] != state["cli_eph"]:
        return "key_exchange"
    n8 = struct.pack(">Q", nonce)
    ready = b"\x05READY" + n8 + _seal(metadata(socket_type, identity), b"CurveZMQREADY---" + n8, state["precom"])
    return ready, {"client_key": client_key, "metadata": meta, "precom": state["precom"]}


# ---- commands sealed under an agreed key ----------------------------------------------------
# A peer that sends a point it holds no secret for (a steered, non-canonical or low-order key:
# tests/hs_steer.py) cannot run X25519 on its side; the key both sides end at is known to the test,
# and these build the peer's commands under that key directly.  Same layouts as above.
def hello_under(k1, cli_eph, nonce=1, box=None):
    """HELLO for the short-term key cli_eph, its box sealed under k1 (or `box`: 80 bytes as they are)"""
    n8 = struct.pack(">Q", nonce)
    if box is None:
        box = _seal(bytes(64), b"CurveZMQHELLO---" + n8, k1)
    assert len(box) == 80 and len(cli_eph) == 32
    return b"\x05HELLO\x01\x00" + bytes(72) + bytes(cli_eph) + n8 + bytes(box)


def welcome_under(k1, srv_eph, cookie96, wnonce):
    """WELCOME: Box [S' + cookie nonce 16 + cookie 80] under k1"""
    assert len(srv_eph) == 32 and len(cookie96) == 96 and len(wnonce) == 16
    return b"\x07WELCOME" + bytes(wnonce) + _seal(bytes(srv_eph) + bytes(cookie96), b"WELCOME-" + bytes(wnonce), k1)


def vouch_under(kv, vouch_nonce, cli_eph, server_key):
    """the vouch Box [C' + S] under kv = beforenm(S', c)"""
    return _seal(bytes(cli_eph) + bytes(server_key), b"VOUCH---" + bytes(vouch_nonce), kv)


def initiate_under(cookie96, precom, plain, nonce=2, box=None):
    """INITIATE: the cookie as received, Box [plain] under precom (or `box`: tag + ciphertext as they are);
    plain = C + vouch nonce + vouch + metadata"""
    n8 = struct.pack(">Q", nonce)
    if box is None:
        box = _seal(plain, b"CurveZMQINITIATE" + n8, precom)
    assert len(cookie96) == 96
    return b"\x08INITIATE" + bytes(cookie96) + n8 + bytes(box)


def ready_under(precom, meta, nonce=1, box=None):
    """READY: Box [metadata] under precom (or `box`: tag + ciphertext as they are)"""
    n8 = struct.pack(">Q", nonce)
    if box is None:
        box = _seal(meta, b"CurveZMQREADY---" + n8, precom)
    return b"\x05READY" + n8 + bytes(box)
