"""The receive rule of a CURVE connection, restated once, and the scenario table every receiver of
this project is run against (tests/test_rx_model.py on the CPU, tests/test_gpu_rx_chain.py on the
device).

The rule is CurveClientMechanism.decode (zmq/io/mechanism/curve/CurveClientMechanism.java:166-224)
and its server twin (CurveServerMechanism.java:165-225), applied in order per connection:

  1. Msgs.startsWith(msg, "MESSAGE", true) (zmq/io/Msgs.java:20-39): size >= 8, byte 0 == 7, bytes
     1..6 == "MESSAG"; its loop ends before byte 7, which is never compared.  Else UNEXPECTED_COMMAND
     (:170-174).
  2. size >= 33, else MALFORMED_COMMAND_MESSAGE (:176-180).
  3. nonce = msg.getLong(8): a signed Java long (:186).
  4. nonce <= cnPeerNonce is rejected (:188-192): INVALID_SEQUENCE on a server
     (CurveServerMechanism.java:188-192), CRYPTOGRAPHIC on a client.
  5. cnPeerNonce = nonce (:193), before the box is opened.
  6. openAfternm (:203); a bad tag is CRYPTOGRAPHIC (:219-223) with cnPeerNonce already moved.
  7. only bits 0 (MORE) and 1 (COMMAND) of the decrypted flags byte reach the Msg (:207-213).

After the first failure StreamEngine.decodeAndPush returns false (StreamEngine.java:1071-1074) and
the engine tears the connection down: nothing more is delivered.  decodeAndPush hands the Msg to
the mechanism whatever flags V2Decoder gave it, so a V2 COMMAND bit on a MESSAGE frame changes
nothing, and V2Decoder takes a LARGE header for any size > 0 (V2Decoder.java:67-105).

Plain Python integers and bytes; payload and tag truth come from the CPU oracle
(cz_testlib.or_curve_decode), never from the library under test.  Nothing is read from the
reference at run time: the line numbers above are citations.
"""
import functools
from collections import namedtuple

from cz_testlib import V2DecoderModel, load_golden, or_curve_decode, or_curve_encode, splitmix_bytes, v2_encode

# include/curvezmq_mi355x.h: CZ_STATUS_*
ST_OK, ST_CRYPTO, ST_MALFORMED, ST_COMMAND, ST_SEQUENCE = 0, 1, 2, 3, 4
STATUS_NAMES = {ST_OK: "OK", ST_CRYPTO: "CRYPTO", ST_MALFORMED: "MALFORMED", ST_COMMAND: "COMMAND",
                ST_SEQUENCE: "SEQUENCE"}
# include/curvezmq_mi355x.h: CZ_ZMTP_* = zmq/ZMQ.java's ZMQ_PROTOCOL_ERROR_ZMTP_*
EV_UNEXPECTED_COMMAND = 0x10000001
EV_INVALID_SEQUENCE = 0x10000002
EV_MALFORMED_COMMAND_MESSAGE = 0x10000012
EV_CRYPTOGRAPHIC = 0x11000001
EVENT_NAMES = {EV_UNEXPECTED_COMMAND: "ZMQ_PROTOCOL_ERROR_ZMTP_UNEXPECTED_COMMAND",
               EV_INVALID_SEQUENCE: "ZMQ_PROTOCOL_ERROR_ZMTP_INVALID_SEQUENCE",
               EV_MALFORMED_COMMAND_MESSAGE: "ZMQ_PROTOCOL_ERROR_ZMTP_MALFORMED_COMMAND_MESSAGE",
               EV_CRYPTOGRAPHIC: "ZMQ_PROTOCOL_ERROR_ZMTP_CRYPTOGRAPHIC"}
CZ_EPROTO, CZ_EMSGSIZE = -71, -90

SERVER, CLIENT = "server", "client"
ROLES = (SERVER, CLIENT)
PRECOM = bytes.fromhex(load_golden()["keys"]["precom"])
M64 = (1 << 64) - 1


def from_server(role):
    """direction of the bodies a receiver of this role opens: a client opens what the server sealed"""
    return 1 if role == CLIENT else 0


def s64(u):
    """an unsigned wire value as the Java long msg.getLong(8) returns"""
    u &= M64
    return u - (1 << 64) if u >> 63 else u


def wire_nonce(body):
    """the big-endian u64 at bytes 8..16 of a body as it lies on the wire"""
    return int.from_bytes(bytes(body[8:16]), "big")


def event_for(status, role):
    if status == ST_COMMAND:
        return EV_UNEXPECTED_COMMAND
    if status == ST_MALFORMED:
        return EV_MALFORMED_COMMAND_MESSAGE
    if status == ST_SEQUENCE:
        return EV_INVALID_SEQUENCE if role == SERVER else EV_CRYPTOGRAPHIC
    return EV_CRYPTOGRAPHIC


def frame_status(body, floor, check, from_srv=0, precom=PRECOM):
    """The per-frame rule the raw kernels implement, with the floor given explicitly.
    Returns (status, flags byte, payload, nonce): all 8 bits of the decrypted flags byte and the
    payload for an accepted frame (else None), the wire nonce once steps 1 and 2 passed (else None)."""
    body = bytes(body)
    if len(body) < 8 or body[0] != 7 or body[1:7] != b"MESSAG":     # step 1
        return ST_COMMAND, None, None, None
    if len(body) < 33:                                               # step 2
        return ST_MALFORMED, None, None, None
    nonce = wire_nonce(body)                                         # step 3
    if check and s64(nonce) <= s64(floor):                           # step 4
        return ST_SEQUENCE, None, None, nonce
    rc, payload, flags, n = or_curve_decode(body, from_srv, precom)  # step 6
    if rc != 0:
        return ST_CRYPTO, None, None, nonce
    assert n == nonce
    return ST_OK, flags, payload, nonce


def chain_expect(bodies, floor0, from_srv, precom=PRECOM):
    """frame_status of every body of a chained raw call: the floor of frame i > 0 is the wire nonce of
    body i - 1, accepted or not"""
    out = []
    for i, b in enumerate(bodies):
        floor = floor0 if i == 0 else wire_nonce(bodies[i - 1])
        out.append(frame_status(b, floor, True, from_srv, precom))
    return out


class RxModel:
    """One connection's receive state: cnPeerNonce and whether the engine has torn it down."""

    def __init__(self, role, cn_peer_nonce, precom=PRECOM):
        assert role in ROLES
        self.role, self.precom = role, precom
        self.peer_nonce = cn_peer_nonce & M64
        self.dead = False
        self.event = 0

    def decode(self, body):
        """(status, event, payload, msg_flags) of the next body; None once the connection is dead"""
        if self.dead:
            return None
        st, flags, payload, nonce = frame_status(body, self.peer_nonce, True, from_server(self.role), self.precom)
        if st in (ST_OK, ST_CRYPTO):
            self.peer_nonce = nonce                                  # step 5, before the tag is known
        if st != ST_OK:
            self.dead = True
            self.event = event_for(st, self.role)
            return st, self.event, None, None
        return ST_OK, 0, payload, flags & 3                          # step 7


Expect = namedtuple("Expect", "delivered peer_nonce status event failed_at")


def sequence_expect(role, cn_peer_nonce, bodies, precom=PRECOM):
    """What a receiver that decodes `bodies` in order ends with: the delivered (payload, flags)
    prefix, cnPeerNonce, and the first failure's status, event and index (status 0, event 0, None)."""
    m = RxModel(role, cn_peer_nonce, precom)
    delivered = []
    for i, b in enumerate(bodies):
        st, ev, payload, fl = m.decode(b)
        if st != ST_OK:
            return Expect(delivered, m.peer_nonce, st, ev, i)
        delivered.append((payload, fl))
    return Expect(delivered, m.peer_nonce, ST_OK, 0, None)


def stream_model(role, cn_peer_nonce, pieces, precom=PRECOM):
    """Wire bytes through V2Decoder and the mechanism, as StreamEngine's inEvent does.  pieces:
    [(bytes, flush)]; after every piece with flush set the whole frames received so far are decoded.
    Returns one dict per flush: `delivered` [(payload, flags)] of that flush, `peer_nonce`, `error`
    (code, event) -- (0, 0) while healthy, (CZ_EPROTO, event) after a mechanism failure, (CZ_EPROTO
    or CZ_EMSGSIZE, 0) after a framing error -- and `refused`: whether later bytes are refused.  A
    mechanism failure ahead of a framing error in the same flush wins.  Bytes for a connection that
    is already refused are dropped."""
    dec, rx = V2DecoderModel(), RxModel(role, cn_peer_nonce, precom)
    stream, done, error, out = b"", 0, (0, 0), []
    for data, flush in pieces:
        if error == (0, 0):
            stream += bytes(data)
            dec.feed(data)
        if not flush:
            continue
        delivered = []
        if error == (0, 0):
            for off, size, _v2flags in dec.msgs[done:]:   # the V2 flags never reach the mechanism
                st, ev, payload, fl = rx.decode(stream[off:off + size])
                if st != ST_OK:
                    error = (CZ_EPROTO, ev)
                    break
                delivered.append((payload, fl))
            done = len(dec.msgs)
            if error == (0, 0) and dec.error:
                error = (CZ_EPROTO if dec.error == "EPROTO" else CZ_EMSGSIZE, 0)
        out.append({"delivered": delivered, "peer_nonce": rx.peer_nonce, "error": error,
                    "refused": error != (0, 0)})
    return out


# ---- the scenario table -----------------------------------------------------------------------
# fault kinds: what is done to one frame of a chain of bodies sealed by the oracle
CUTS = {"cut32": 32, "cut16": 16, "cut8": 8, "cut7": 7, "cut0": 0, "name_short20": 20}
FAULT_KINDS = ("tag", "ct_last", "wrong_dir", "name3", "name7", "cut32", "cut16", "cut8", "cut7", "cut0",
               "replay", "replay_tag", "name_short20", "flags_ff")
# what the first frame carrying the fault must give (the frames before it are valid)
FAULT_STATUS = {"tag": ST_CRYPTO, "ct_last": ST_CRYPTO, "wrong_dir": ST_CRYPTO, "name3": ST_COMMAND, "name7": ST_OK,
                "cut32": ST_MALFORMED, "cut16": ST_MALFORMED, "cut8": ST_MALFORMED, "cut7": ST_COMMAND,
                "cut0": ST_COMMAND, "replay": ST_SEQUENCE, "replay_tag": ST_SEQUENCE, "name_short20": ST_COMMAND,
                "flags_ff": ST_OK}
UNIFORM_KINDS = ("tag", "ct_last", "wrong_dir", "name3", "name7", "replay", "replay_tag", "flags_ff")  # keep the size
POSITIONS = ("0", "1", "63", "64", "65", "last")
CHAIN_LENGTHS = (1, 64, 65, 130)
BODY_SIZES = (33, 34, 96, 97, 161, 4129, 300033)
BIG = 300033
UNIFORM_SIZES = (34, 161, 4129)
CARRY_FRAMES = 1024      # 8-byte strides of a 4129-byte body repeat their line phase every 16 frames: one
#                          block of the phase-sorted kernel is 64 x 16 frames, the tail follows it
# nonce runs, as unsigned wire values: (floor, nonces, per-frame statuses)
NONCE_RUNS = {
    "gaps_equal_back": (2, (3, 4, 9, 1000, 1000, 999), (0, 0, 0, 0, ST_SEQUENCE, ST_SEQUENCE)),
    "around_2_32": ((1 << 32) - 2, ((1 << 32) - 1, 1 << 32, (1 << 32) + 1), (0, 0, 0)),
    "into_negative": ((1 << 63) - 2, ((1 << 63) - 1, 1 << 63), (0, ST_SEQUENCE)),
    "wrap": (1 << 63, ((1 << 63) + 1, (1 << 64) - 1, 0, 1), (0, 0, 0, 0)),
}

Frame = namedtuple("Frame", "nonce size fault flags seed")


def build_body(fr, role, precom=PRECOM):
    """one frame's wire body: sealed by the oracle for the direction `role` opens, then damaged"""
    fs = from_server(role) ^ (1 if fr.fault == "wrong_dir" else 0)
    flags = 0xff if fr.fault == "flags_ff" else fr.flags
    body = bytearray(or_curve_encode(splitmix_bytes(fr.size - 33, fr.seed), flags, fr.nonce & M64, fs, precom))
    if fr.fault in ("tag", "replay_tag"):
        body[16] ^= 1
    elif fr.fault == "ct_last":
        body[-1] ^= 0x80
    elif fr.fault in ("name3", "name_short20"):
        body[3] ^= 0x20
    elif fr.fault == "name7":
        body[7] ^= 0x55
    if fr.fault in CUTS:
        body = body[:CUTS[fr.fault]]
    return bytes(body)


class Scenario:
    """A chain of frames of one connection.  floor: cnPeerNonce before frame 0 (unsigned).
    uniform: the common body size when every body has it (cz_open_uniform takes those), else None.
    tags: what the coverage condition counts -- ("fault", kind, position), ("run", name), ("len", n)."""

    def __init__(self, name, floor, frames, tags=(), uniform=None):
        self.name, self.floor, self.frames, self.tags, self.uniform = name, floor & M64, tuple(frames), tuple(tags), uniform

    def __repr__(self):
        return f"Scenario({self.name}, {len(self.frames)} frames)"

    def bodies(self, role):
        return _bodies(self, role)

    def payload(self, i):
        return splitmix_bytes(self.frames[i].size - 33, self.frames[i].seed)

    def raw_count(self, role):
        """frames a chained raw call takes: a body under 16 bytes has no whole nonce for its successor's
        floor, so it is only ever the last frame"""
        for i, b in enumerate(self.bodies(role)):
            if len(b) < 16:
                return i + 1
        return len(self.frames)

    def expect(self, role):
        return _expect(self, role)

    def raw_expect(self, role):
        return _raw_expect(self, role)

    def wire(self, role):
        return b"".join(v2_encode(b) for b in self.bodies(role))

    def faults(self):
        return [i for i, f in enumerate(self.frames) if f.fault]


@functools.lru_cache(maxsize=None)
def _bodies(sc, role):
    return tuple(build_body(f, role) for f in sc.frames)


@functools.lru_cache(maxsize=None)
def _expect(sc, role):
    return sequence_expect(role, sc.floor, sc.bodies(role))


@functools.lru_cache(maxsize=None)
def _raw_expect(sc, role):
    return tuple(chain_expect(sc.bodies(role)[:sc.raw_count(role)], sc.floor, from_server(role)))


_SMALL = (34, 96, 97, 161, 33)


def _chain(floor, count, seed, size_of=None):
    """count valid frames above `floor`: nonces rise by 1 or 2, sizes cycle, flags cycle 0..3"""
    frames, n = [], floor
    for i in range(count):
        n = (n + 1 + (1 if i % 3 == 0 else 0)) & M64
        size = size_of(i) if size_of else (4129 if i % 41 == 7 else _SMALL[i % len(_SMALL)])
        frames.append(Frame(n, size, None, i & 3, seed * 1000 + i))
    return frames


def _set_fault(frames, floor, p, kind, size=None):
    f = frames[p]
    nonce = f.nonce
    if kind in ("replay", "replay_tag"):                 # the nonce of the frame before it, or the floor
        nonce = frames[p - 1].nonce if p else floor
    frames[p] = Frame(nonce, size or f.size, kind, f.flags, f.seed)


@functools.lru_cache(maxsize=None)
def scenarios():
    """The table; deterministic, nothing random.  One fault per grid scenario, every kind at every
    position; the nonce runs; the 300 033-byte body accepted and rejected in every way; and uniform
    chains (one size, several faults and all runs in one chain) for the raw per-frame receivers."""
    out = []
    fault_sizes = (33, 34, 96, 97, 161, 4129)
    lengths = {"0": (1, 64, 65, 130), "1": (64, 65, 130), "63": (64, 65, 130), "64": (65, 130), "65": (130,),
               "last": (130, 65, 64, 1)}
    for k, kind in enumerate(FAULT_KINDS):
        for q, pos in enumerate(POSITIONS):
            count = lengths[pos][k % len(lengths[pos])]
            p = count - 1 if pos == "last" else int(pos)
            floor = (2, 1, (1 << 32) - 5, (1 << 63) + 7, (1 << 64) - 50)[(k + q) % 5]   # none crosses 2^63 - 1
            frames = _chain(floor, count, 100 + 10 * k + q)
            _set_fault(frames, floor, p, kind, fault_sizes[(k + q) % len(fault_sizes)])
            tags = [("fault", kind, pos), ("len", count)]
            if p == count - 1:
                tags.append(("fault", kind, "last"))
            if str(p) in POSITIONS:
                tags.append(("fault", kind, str(p)))
            out.append(Scenario(f"{kind}@{pos}/{count}", floor, frames, tags))
    for name, (floor, nonces, _st) in NONCE_RUNS.items():
        frames = [Frame(n, _SMALL[i % len(_SMALL)], None, i & 3, 7000 + i) for i, n in enumerate(nonces)]
        out.append(Scenario(f"run:{name}", floor, frames, [("run", name)]))
    # the body the segment planners split: accepted with its successor's floor read from it, and
    # rejected early (SEQUENCE, COMMAND) and by its tag
    for name, kind, after in (("ok_then_next", None, None), ("ok_then_replay_of_it", None, "replay"),
                              ("replay", "replay", None), ("name3", "name3", None), ("tag", "tag", None),
                              ("ct_last", "ct_last", None)):
        frames = _chain(2, 4, 9000 + len(out))
        frames[1] = frames[1]._replace(size=BIG)
        if kind:
            _set_fault(frames, 2, 1, kind)
        if after:
            _set_fault(frames, 2, 2, after)
        out.append(Scenario(f"big:{name}", 2, frames, [("big", name)]))
    frames = _chain(5, 2, 9900)
    frames[0] = frames[0]._replace(size=BIG)
    _set_fault(frames, 5, 0, "replay")
    out.append(Scenario("big:replay@0", 5, frames, [("big", "replay@0")]))
    for size in UNIFORM_SIZES:
        for rot in range(3):
            out.append(_uniform_chain(size, 130, rot))
    out.append(_uniform_chain(4129, CARRY_FRAMES + 130, 1, tail=CARRY_FRAMES))
    names = [s.name for s in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def _uniform_chain(size, count, rot, tail=None):
    """One size, per-frame semantics: frames 0..6 carry negative nonces above a negative floor, frame 7
    is 2, then the four nonce runs back to back (each run's floor is the frame before it), then small
    rising nonces; faults that keep the size at 0, 1, 63, 64, 65 and the last frame (kinds rotated by
    `rot`), and with `tail` one on the first frame behind the phase-sorted block and two inside it."""
    floor = (1 << 63) + 5
    nonces = [(1 << 63) + 6 + i for i in range(7)]
    for f0, run, _st in NONCE_RUNS.values():
        if nonces[-1] != f0:         # ("into_negative" ends on the floor of "wrap")
            nonces.append(f0)
        nonces.extend(run)
    n = 10
    while len(nonces) < count:
        n += 1 + (len(nonces) % 2)
        nonces.append(n)
    frames = [Frame(nonces[i], size, None, i & 3, 50000 + size * 7 + i) for i in range(count)]
    tags = [("uniform", size), ("len", count)]
    spots = [0, 1, 63, 64, 65, count - 1] + ([tail, tail - 1, 500] if tail else [])
    for j, p in enumerate(spots):
        kind = UNIFORM_KINDS[(j + 3 * rot) % len(UNIFORM_KINDS)]
        _set_fault(frames, floor, p, kind)
        tags.append(("uniform_fault", kind, p))
    return Scenario(f"uniform{size}x{count}r{rot}", floor, frames, tags, uniform=size)


def single_fault_scenarios():
    """the scenarios that are not uniform chains: at most one damaged frame each"""
    return tuple(s for s in scenarios() if s.uniform is None)
