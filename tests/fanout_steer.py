"""Inputs for the PUB fan-out edge tests: steered payloads and flush scenarios.  No device.

Steered cases.  A fan-out launch seals ONE payload for many subscribers; the ciphertext of
subscriber i is payload ^ keystream(key_i, counter_i), so one payload can be steered (poly_steer.py)
for exactly one (key, counter) pair: that subscriber's Poly1305 accumulator ends at the chosen
residue, every other lane sees an ordinary message.  steered_case() builds the payload and the body
the steered subscriber must get, tag from the big-integer poly_steer.poly1305, and asserts while
building that the oracle reproduces it.

Flush scenarios.  cz_engine_flush_out cuts a flush of 16 MiB or more of wire bytes into groups;
flush_groups() restates the documented rule for one purpose only, to choose the traffic of
tests/test_gpu_fanout_edges.py and to prove (tests/test_fanout_steer.py) that the group edges fall
where the scenarios' names say.  No GPU assertion depends on it: what a flush must put on the wire
is the oracle's seal of each connection's messages in send order, wherever the edges are.
Helper module of test_fanout_steer.py and test_gpu_fanout_edges.py.
"""
import functools
import random
from collections import namedtuple

import numpy as np

import poly_steer as ps
from cz_testlib import or_curve_encode, splitmix_bytes, splitmix_words

# ---- steered fan-out cases ------------------------------------------------------------------------
# payload lengths (the MAC covers n + 1 bytes): 31 the shortest steerable, 31/32 and 46/47 around
# two and three MAC blocks, 95/96 around two box blocks, 223 the smallest body (256 bytes) that
# pick_staging gives to ST_LINES and 224 the first past it, 4063 an odd block count for the pair loop
FAN_LENS = [31, 32, 46, 47, 95, 96, 223, 224, 4063]
EDGE_COUNTERS = [(1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 2, 0x0000_0123_4567_89AB]
# the key table of the kernel tests: entry t is precom t % NPRE under direction t // NPRE
# (0: C2S, 1: S2C), so one table mixes both directions' subkeys
NPRE = 12
PRECOMS = splitmix_words(NPRE * 4, 0xFA57).view(np.uint8).copy()   # NPRE x 32 bytes

Case = namedtuple("Case", "name key_idx direction counter flags payload body tag")


def precom(k):
    return PRECOMS[32 * k:32 * k + 32].tobytes()


def specs(n):
    """what a payload of n bytes is steered to: every final target of ps.TARGETS, and from three MAC
    blocks up the two h + m ripples -- tests/test_gpu_poly_edges.py::_specs"""
    out = [(name, f, None) for name, f in ps.TARGETS]
    if n + 1 >= 48:
        out += [(f"h+m-ripple-{x}", None, x) for x in (0, 3)]
    return out


def _xor(a, b):
    assert len(a) == len(b)
    return (int.from_bytes(a, "little") ^ int.from_bytes(b, "little")).to_bytes(len(a), "little")


def steered_case(precom32, direction, counter, flags, n, spec, rng):
    """(payload, body): the n-byte payload whose seal under (precom32, direction, counter) with the
    flags byte `flags` has its Poly1305 accumulator steered to `spec`, and that seal.  Nothing is
    caught: ps.steer raises when it cannot solve."""
    name, f, x = spec
    ks = ps.message_keystream(precom32, direction, counter, 33 + n)
    key, head = ks[:32], bytes([ks[32] ^ flags])
    if f is not None:
        msg = ps.steer(key, n + 1, f(ps.key_s(key)), rng, head)
    else:
        msg = ps.hm_ripple(key, n + 1, x, rng, head)
    plain = _xor(msg, ks[32:])
    assert plain[0] == flags, name
    payload = plain[1:]
    body = b"\x07MESSAGE" + counter.to_bytes(8, "big") + ps.poly1305(msg, key) + msg
    assert or_curve_encode(payload, flags, counter, direction, precom32) == body, name
    return payload, body


@functools.lru_cache(maxsize=None)
def cases(n):
    """One Case per spec at payload length n.  The steered subscriber's direction cycles over C2S and
    S2C, its counter over EDGE_COUNTERS (2 and 5 are coprime: every pair occurs), flags over 0..3."""
    rng = random.Random(4000 + n)
    out = []
    for j, spec in enumerate(specs(n)):
        direction, counter, flags, k = j % 2, EDGE_COUNTERS[j % len(EDGE_COUNTERS)], (j // 2) % 4, (5 * j + n) % NPRE
        payload, body = steered_case(precom(k), direction, counter, flags, n, spec, rng)
        out.append(Case(spec[0], direction * NPRE + k, direction, counter, flags, payload, body, body[16:32]))
    return out


def round_up(v, a):
    return (v + a - 1) // a * a


# output layouts of the kernel tests: name -> stride(mlen), or None where the layout has no stride
# for that length by construction
def stride_slots128(mlen):
    return round_up(mlen, 128)


def stride_region16(mlen):
    s = round_up(mlen, 16)
    return s if s <= 256 and s % 128 else None


def stride_dense_unaligned(mlen):
    return mlen + 7


LAYOUTS = {"slots128": stride_slots128, "region16": stride_region16, "dense_unaligned": stride_dense_unaligned}


def layout_cases():
    """(length, layout) pairs: the lengths with no region16 stride are left out here, not at run time"""
    return [(n, name) for name, f in LAYOUTS.items() for n in FAN_LENS if f(n + 33) is not None]


def census():
    """{length: [spec names]} of the cases that exist, and {layout: [lengths]}"""
    return {n: [c.name for c in cases(n)] for n in FAN_LENS}, {name: [n for n, l in layout_cases() if l == name]
                                                                 for name in LAYOUTS}


# ---- the flush-group rule ----------------------------------------------------------------------------
GROUP_BYTES = 8 << 20
MAX_GROUPS = 16


def frame_wire_bytes(length):
    body = length + 33
    return body + (9 if body > 255 else 2)


def flush_groups(payload_lens):
    """[(first, end)] frame ranges of a flush of these payloads in send order: w wire bytes give
    G = min(16, max(1, w // 8 MiB)) groups, and group g closes at the first frame whose end position
    times G is at least w (g + 1)"""
    pos, w = [], 0
    for n in payload_lens:
        w += frame_wire_bytes(n)
        pos.append(w)
    G = min(MAX_GROUPS, max(1, w // GROUP_BYTES))
    groups, first = [], 0
    for i, end in enumerate(pos):
        if i + 1 == len(pos) or end * G >= w * (len(groups) + 1):
            groups.append((first, i + 1))
            first = i + 1
    return groups


# ---- flush scenarios ---------------------------------------------------------------------------------
# ops, over connection indices 0..ncon-1 and payload names:
#   ("alloc", name)                         cz_engine_msg_alloc a buffer and fill it with the payload; a
#                                           later send / publish of that name goes out in place
#   ("send", conn, name, more, command)
#   ("publish", [conns], name, more, command)
Frame = namedtuple("Frame", "conn name flags pub")   # pub: 1-based index of the publish op, 0 for a send
NCON = 520
SEND_CONNS = (5, 77, 300)


class Scenario:
    def __init__(self, name, payloads, ops, ncon=NCON):
        self.name, self.payloads, self.ops, self.ncon = name, payloads, ops, ncon

    def frames(self):
        out, pub = [], 0
        for op in self.ops:
            if op[0] == "send":
                out.append(Frame(op[1], op[2], (1 if op[3] else 0) | (2 if op[4] else 0), 0))
            elif op[0] == "publish":
                pub += 1
                out += [Frame(c, op[2], (1 if op[3] else 0) | (2 if op[4] else 0), pub) for c in op[1]]
        return out

    def groups(self):
        return flush_groups([len(self.payloads[f.name]) for f in self.frames()])


def _sends(count, seed):
    """`count` sends of 8192 bytes spread over SEND_CONNS, every payload its own"""
    pay = {f"s{seed}-{j}": splitmix_bytes(8192, 9000 + 16 * seed + j) for j in range(count)}
    return pay, [("send", SEND_CONNS[j % len(SEND_CONNS)], name, False, False) for j, name in enumerate(pay)]


SWEEP_K = [0, 1, 3, 4, 5]   # frames of the split publish on the short side of the edge, around fanout_min 4
SWEEP_FANOUT_MIN = 4


@functools.lru_cache(maxsize=None)
def edge_sweep(side, k):
    """Four publishes of 8192 bytes to all 520 connections (four payloads, the second with MORE) and
    2 k sends of 8192 bytes behind them ("trailing": the one group edge lies k frames into the third
    publish) or in front ("leading": k frames before the end of the second)."""
    pay = {f"p{j}": splitmix_bytes(8192, 8100 + j) for j in range(4)}
    pubs = [("publish", list(range(NCON)), f"p{j}", j == 1, False) for j in range(4)]
    spay, sends = _sends(2 * k, 1 if side == "trailing" else 2)
    pay.update(spay)
    return Scenario(f"{side}-{k}", pay, pubs + sends if side == "trailing" else sends + pubs)


@functools.lru_cache(maxsize=None)
def two_edges():
    """One publish of 8192 bytes to a list of 3300 entries, the 520 ids repeated in a shuffled order
    (an id named several times gets consecutive nonces): three groups, the publish split twice"""
    rng = random.Random(3300)
    ids = [i % NCON for i in range(3300)]
    rng.shuffle(ids)
    return Scenario("two-edges", {"p": splitmix_bytes(8192, 8200)}, [("publish", ids, "p", False, False)])


MIXED_LENS = {"e": 0, "h": 100, "l": 223, "b": 65536}
MIXED_LISTS = [3, 63, 64, 65, 520]
IOV_CONNS = (7, 11)   # these two get sends between the publishes: their frames interleave with others'


@functools.lru_cache(maxsize=None)
def mixed():
    """Every publish length of MIXED_LENS to every list size of MIXED_LISTS (20 publishes in a
    shuffled order, each list a sorted sample of the connections), sends of other sizes between them
    on connections 7, 11 and 300, and one send whose payload is msg_alloc'ed before everything and
    queued after: the arena is out of send order."""
    rng = random.Random(65)
    pay = {name: splitmix_bytes(n, 8300 + n) for name, n in MIXED_LENS.items()}
    sizes = [300, 4096, 17, 70000, 1, 255, 5000, 222, 31, 9000]
    pay.update({f"s{j}": splitmix_bytes(n, 8400 + j) for j, n in enumerate(sizes)})
    pay["early"] = splitmix_bytes(1000, 8500)
    pubs = [(name, size) for name in MIXED_LENS for size in MIXED_LISTS]
    rng.shuffle(pubs)
    ops = [("alloc", "early")]
    for j, (name, size) in enumerate(pubs):
        ids = list(range(NCON)) if size == NCON else sorted(rng.sample(range(NCON), size))
        if j % 2 == 0:
            s = j // 2
            ops.append(("send", (7, 11, 300)[s % 3], f"s{s}", s % 4 == 1, False))
        ops.append(("publish", ids, name, j % 5 == 2, False))
    ops.append(("send", 7, "early", False, False))
    return Scenario("mixed", pay, ops)


def scenarios():
    return ([edge_sweep(side, k) for side in ("trailing", "leading") for k in SWEEP_K] + [two_edges(), mixed()])
