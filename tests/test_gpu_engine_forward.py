"""GPU: the engine's forward routes (cz_engine_forward / cz_engine_flush_forward) between real engines.

Two engines are the peers (64 client connections each) and one is the broker, with the 64 routed pairs
A_i -> B_i and B_i -> A_i.  What a source peer sends arrives, re-sealed by the broker without delivery, at the
destination peer, whose flush_in is the judge.  The second yardstick is a second broker that takes the same bytes
through flush_in + send + flush_out: same wire bytes when nothing is rejected, same nonces at all four ends,
same error and event for a tampered frame."""
import pytest

import rx_model as rx
from cz_testlib import splitmix_bytes

pytestmark = pytest.mark.gpu

NPAIR = 64
PRE_A, PRE_B = rx.PRECOM, splitmix_bytes(32, 4243)
SIZES = (0, 1, 100, 222, 223, 300, 4096)      # 222 / 223: the body at the 2-byte to 9-byte header edge


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from jeromq_amd import _lib
    return _lib


class World:
    """peers pa / pb (clients a[i] / b[i]), the broker br with servers A[i] / B[i] routed both ways, the second
    broker br2 with the same connections and no route, and its own destination peers pa2 / pb2"""

    def __init__(self, extra=0):
        from jeromq_amd.engine import CurveBatchEngine
        self.engines = [CurveBatchEngine(arena_bytes=1 << 22) for _ in range(6)]
        self.pa, self.pb, self.br, self.br2, self.pa2, self.pb2 = self.engines
        n = NPAIR + extra
        self.a, self.a2 = (e.add_connections([PRE_A] * n, as_server=False) for e in (self.pa, self.pa2))
        self.b, self.b2 = (e.add_connections([PRE_B] * n, as_server=False) for e in (self.pb, self.pb2))
        self.A, self.B = self.br.add_connections([PRE_A] * n, as_server=True), self.br.add_connections([PRE_B] * n, as_server=True)
        assert self.br2.add_connections([PRE_A] * n, as_server=True) == self.A
        assert self.br2.add_connections([PRE_B] * n, as_server=True) == self.B
        for i in range(NPAIR):
            self.br.forward(self.A[i], self.B[i])
            self.br.forward(self.B[i], self.A[i])

    def close(self):
        for e in self.engines:
            e.close()


@pytest.fixture()
def world(gpu):
    w = World(extra=3)
    yield w
    w.close()


def _msgs(i, rnd, side):
    """connection i's multipart message of a round: 1..4 parts, MORE on all but the last"""
    n = 1 + (i + rnd) % 4
    return [(splitmix_bytes(SIZES[(i + 3 * k + rnd + side) % len(SIZES)], 9000 * rnd + 100 * i + 10 * side + k), k + 1 < n)
            for k in range(n)]


def _send(peer, conns, rnd, side):
    """every connection of a peer sends its message of the round -> {i: wire}, {i: [(payload, flags)]}"""
    sent = {}
    for i in range(NPAIR):
        sent[i] = [(p, 1 if more else 0) for p, more in _msgs(i, rnd, side)]
        for p, more in _msgs(i, rnd, side):
            assert peer.send(conns[i], p, more=more) == 0
    peer.flush_out()
    return {i: peer.wire_out(conns[i]) for i in range(NPAIR)}, sent


def _second_broker(w, src, dst, wires):
    """the same bytes through flush_in + send + flush_out -> {i: wire for the destination}"""
    for i, wire in wires.items():
        assert w.br2.recv(src[i], wire) == 0
    w.br2.flush_in()
    for i in wires:
        for payload, fl in w.br2.messages_in(src[i]):
            w.br2.send(dst[i], payload, more=bool(fl & 1), command=bool(fl & 2))
    w.br2.flush_out()
    return {i: w.br2.wire_out(dst[i]) for i in wires}


def test_multipart_messages_pass_both_ways_like_through_the_second_broker(world):
    w, bad = world, []
    for rnd in range(2):
        wa, sent_a = _send(w.pa, w.a, rnd, 0)
        wb, sent_b = _send(w.pb, w.b, rnd, 1)
        for i in range(NPAIR):
            assert w.br.recv(w.A[i], wa[i]) == 0 and w.br.recv(w.B[i], wb[i]) == 0
        w.br.flush_in()                                     # a routed connection yields no msgs_in: its bytes wait
        assert all(w.br.messages_in(c) == [] for c in w.A[:NPAIR] + w.B[:NPAIR])
        w.br.flush_forward()
        assert w.br.forward_frames == sum(len(m) for m in sent_a.values()) + sum(len(m) for m in sent_b.values())
        out_ab = {i: w.br.forward_out(w.A[i]) for i in range(NPAIR)}
        out_ba = {i: w.br.forward_out(w.B[i]) for i in range(NPAIR)}
        ref_ab, ref_ba = _second_broker(w, w.A, w.B, wa), _second_broker(w, w.B, w.A, wb)
        for i in range(NPAIR):
            if out_ab[i] != ref_ab[i] or out_ba[i] != ref_ba[i]:
                bad.append(f"round {rnd} pair {i}: the forwarded bytes differ from the second broker's wire_out")
            for peer, conn, data in ((w.pb, w.b[i], out_ab[i]), (w.pa, w.a[i], out_ba[i]),
                                     (w.pb2, w.b2[i], ref_ab[i]), (w.pa2, w.a2[i], ref_ba[i])):
                assert peer.recv(conn, data) == 0
        for e in (w.pa, w.pb, w.pa2, w.pb2):
            e.flush_in()
        for i in range(NPAIR):
            if w.pb.messages_in(w.b[i]) != sent_a[i] or w.pa.messages_in(w.a[i]) != sent_b[i]:
                bad.append(f"round {rnd} pair {i}: the destination peer did not get what the source peer sent")
            ends = [(w.br.nonce(c), w.br.peer_nonce(c), w.br.error(c)) for c in (w.A[i], w.B[i])]
            ends2 = [(w.br2.nonce(c), w.br2.peer_nonce(c), w.br2.error(c)) for c in (w.A[i], w.B[i])]
            peers = [(e.nonce(c), e.peer_nonce(c), e.error(c)) for e, c in ((w.pa, w.a[i]), (w.pb, w.b[i]))]
            peers2 = [(e.peer_nonce(c), e.error(c)) for e, c in ((w.pa2, w.a2[i]), (w.pb2, w.b2[i]))]
            if ends != ends2 or [(p[1], p[2]) for p in peers] != peers2:
                bad.append(f"round {rnd} pair {i}: nonces {ends} {peers}, through the second broker {ends2} {peers2}")
            if peers[0][1] != ends[0][0] - 1 or peers[1][1] != ends[1][0] - 1:
                bad.append(f"round {rnd} pair {i}: the peers' cnPeerNonce is not the broker's last outbound nonce")
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("cut", ["header", "large_header", "body"])
def test_a_partial_frame_is_forwarded_after_its_second_half(world, cut):
    w = world
    wa, sent_a = _send(w.pa, w.a, 2, 0)             # round 2: pair i sends 1 + (i + 2) % 4 parts
    ref = _second_broker(w, w.A, w.B, wa)
    from jeromq_amd import wire as W
    first = {}
    for i in range(NPAIR):
        frames, _c, _rc = W.parse(wa[i])
        k = len(frames) // 2                        # the frame that is split
        start = int(frames[k - 1]["body_off"]) + int(frames[k - 1]["size"]) if k else 0
        body = int(frames[k]["body_off"])
        at = {"header": start + 1, "large_header": start + (5 if body - start == 9 else 1),
              "body": body + int(frames[k]["size"]) // 2 + 1}[cut]
        first[i] = (at, start)
        assert 0 < at < len(wa[i])
        assert w.br.recv(w.A[i], wa[i][:at]) == 0
    w.br.flush_forward()
    part1 = {i: w.br.forward_out(w.A[i]) for i in range(NPAIR)}
    for i in range(NPAIR):
        assert part1[i] == ref[i][:first[i][1]], f"pair {i}: the whole frames before the split, and nothing of it"
        assert w.br.error(w.A[i]) == (0, 0)
        assert w.br.recv(w.A[i], wa[i][first[i][0]:]) == 0
    w.br.flush_forward()
    for i in range(NPAIR):
        assert part1[i] + w.br.forward_out(w.A[i]) == ref[i], f"pair {i}"
        assert (w.br.nonce(w.B[i]), w.br.peer_nonce(w.A[i])) == (w.br2.nonce(w.B[i]), w.br2.peer_nonce(w.A[i]))
        assert w.pb.recv(w.b[i], ref[i]) == 0
    w.pb.flush_in()
    assert all(w.pb.messages_in(w.b[i]) == sent_a[i] for i in range(NPAIR))


def test_a_tampered_frame_fails_only_its_source(world):
    w = world
    from jeromq_amd import wire as W
    wa, sent_a = _send(w.pa, w.a, 3, 0)             # round 3: pair i sends 1 + (i + 3) % 4 parts
    wb, sent_b = _send(w.pb, w.b, 3, 1)
    victim = next(i for i in range(NPAIR) if len(sent_a[i]) == 4)
    frames, _c, _rc = W.parse(wa[victim])
    bad_wire = bytearray(wa[victim])
    bad_wire[int(frames[2]["body_off"]) + 16] ^= 0x10       # a tag bit of the third frame
    wa[victim] = bytes(bad_wire)
    before = w.br.nonce(w.B[victim])
    for i in range(NPAIR):
        assert w.br.recv(w.A[i], wa[i]) == 0 and w.br2.recv(w.A[i], wa[i]) == 0
    w.br.flush_forward()
    w.br2.flush_in()
    end2 = int(frames[1]["body_off"]) + int(frames[1]["size"])
    out = w.br.forward_out(w.A[victim])
    assert len(out) == end2 and out[:2] == wa[victim][:2], "the bytes before the rejected frame leave, nothing after"
    assert w.br.forward_frames == sum(len(m) for m in sent_a.values()) - 2
    for i in range(NPAIR):
        assert w.br.error(w.A[i]) == w.br2.error(w.A[i]) == ((rx.CZ_EPROTO, rx.EV_CRYPTOGRAPHIC) if i == victim else (0, 0))
        assert w.br.peer_nonce(w.A[i]) == w.br2.peer_nonce(w.A[i])
        assert w.br.error(w.B[i]) == (0, 0)
        assert w.pb.recv(w.b[i], w.br.forward_out(w.A[i])) == 0
    assert w.br.nonce(w.B[victim]) == before + 4, "every scanned frame consumed a counter"
    w.pb.flush_in()
    for i in range(NPAIR):
        assert w.pb.messages_in(w.b[i]) == (sent_a[i][:2] if i == victim else sent_a[i]) and w.pb.error(w.b[i]) == (0, 0)
    assert w.br.recv(w.A[victim], wa[victim]) == rx.CZ_EPROTO          # the failed source refuses more bytes
    # a route whose destination has failed leaves the source's bytes where they are and forwards nothing
    for i in range(NPAIR):
        assert w.br.recv(w.B[i], wb[i]) == 0
    held = w.br.peer_nonce(w.B[victim])
    w.br.flush_forward()
    assert w.br.forward_out(w.B[victim]) == b"" and w.br.peer_nonce(w.B[victim]) == held
    assert w.br.error(w.B[victim]) == (0, 0)
    for i in range(NPAIR):
        if i != victim:
            assert w.pa.recv(w.a[i], w.br.forward_out(w.B[i])) == 0
    w.pa.flush_in()
    assert all(w.pa.messages_in(w.a[i]) == sent_b[i] for i in range(NPAIR) if i != victim)
    # ... and once that route is cleared they are delivered by flush_in
    w.br.forward(w.B[victim], None)
    w.br.flush_in()
    assert w.br.messages_in(w.B[victim]) == sent_b[victim]


def test_routes_are_checked_and_an_unrouted_connection_is_still_served(world, gpu):
    w, L = world, gpu
    f = L.lib().cz_engine_forward
    h = w.br._h
    u, x, y = NPAIR, NPAIR + 1, NPAIR + 2           # the three extra pairs: never routed by World
    assert f(h, w.A[u], w.B[0]) == L.CZ_EINVAL      # a destination another route names
    assert f(h, w.A[u], w.A[u]) == L.CZ_EINVAL      # from == to
    assert f(h, w.A[u], 100000) == L.CZ_EINVAL and f(h, -1, w.A[u]) == L.CZ_EINVAL and f(h, w.A[u], -2) == L.CZ_EINVAL
    assert f(h, w.A[0], w.B[0]) == L.CZ_OK          # the same route again
    w.br.forward(w.A[x], w.A[y])
    w.br.remove_connection(w.A[y])                  # removing the destination clears the route ...
    assert f(h, w.A[x], w.A[y]) == L.CZ_EINVAL and f(h, w.A[y], w.A[x]) == L.CZ_EINVAL      # ... and the id is gone
    w.br.forward(w.B[x], w.B[y])
    w.br.remove_connection(w.B[x])                  # removing the source clears it too: B[y] is free again
    w.br.forward(w.B[u], w.B[y])
    w.br.forward(w.B[u], None)
    # traffic: pair 0 routed, A[u] and A[x] unrouted on the same engine
    msgs = {c: [(splitmix_bytes(50 + c, c), 1), (splitmix_bytes(300, c + 1), 0)] for c in (0, u, x)}
    for c, m in msgs.items():
        for p, more in m:
            w.pa.send(w.a[c], p, more=bool(more))
    w.pa.flush_out()
    for c in msgs:
        assert w.br.recv(w.A[c], w.pa.wire_out(w.a[c])) == 0
    w.br.flush_in()
    assert w.br.messages_in(w.A[u]) == msgs[u] and w.br.messages_in(w.A[x]) == msgs[x]
    assert w.br.messages_in(w.A[0]) == [] and w.br.forward_out(w.A[0]) == b""
    w.br.flush_forward()
    assert w.br.forward_frames == 2 and w.br.forward_out(w.A[u]) == b""
    assert w.pb.recv(w.b[0], w.br.forward_out(w.A[0])) == 0
    w.pb.flush_in()
    assert w.pb.messages_in(w.b[0]) == msgs[0]
    w.br.flush_forward()                            # nothing received: nothing forwarded
    assert w.br.forward_frames == 0 and w.br.forward_out(w.A[0]) == b""
