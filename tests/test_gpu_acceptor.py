"""GPU: the batched CURVE server handshake (jeromq_amd.acceptor, cz_acceptor.cpp, cz_accept_kernels.h).

Yardsticks: the libzmq 4.3.4 server session of tests/golden/libzmq_session.json, the CPU model of
tests/hs_model.py (anchored to libzmq by tests/test_hs_model.py) and, where the issue is what the
per-connection state machine does with a command, a CurveServerHandshake (cz_hs) fed the same bytes.
Shapes are the smallest at which the lane-per-connection kernels can go wrong: one lane, two full
64-lane workgroups plus a tail, every INITIATE length, and batches whose lanes take different paths."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import hs_model as M
from cz_testlib import or_beforenm, splitmix_bytes, v2_encode

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
S = json.load(open(os.path.join(HERE, "golden", "libzmq_session.json")))
CLIENT_PUB = bytes.fromhex("BB88471D65E2659B30C55A5321CEBB5AAB2B70A398645C26DCA2B2FCB43FC518")
CLIENT_SEC = bytes.fromhex("7BB864B489AFA3671FBE69101F94B38972F24816DFB01B51656B3FEC8DFD0888")
SERVER_PUB = bytes.fromhex("54FCBA24E93249969316FB617C872BB0C1D1FF14800427C594CBFACF1BC2D652")
SERVER_SEC = bytes.fromhex("8E0BDD697628B91D8F245587EE95C5B04D48963F79259877B49CD9063AEAD3B7")

UNEXPECTED, MALFORMED_HELLO, MALFORMED_INITIATE = 0x10000001, 0x10000013, 0x10000014
CRYPTOGRAPHIC, KEY_EXCHANGE = 0x11000001, 0x10000003
ZMQ_PAIR, ZMQ_PUB, ZMQ_SUB, ZMQ_DEALER, ZMQ_ROUTER = 0, 1, 2, 5, 6


def H(x):
    return bytes.fromhex(x)


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from jeromq_amd import _lib, acceptor, engine, handshake
    return type("G", (), {"lib": _lib, "acceptor": acceptor, "engine": engine, "hs": handshake})


@functools.lru_cache(maxsize=None)
def conn(i, seed):
    """connection i of a test: the client's long-term and short-term secrets, the server's short-term
    secret and entropy, the vouch nonce -- all distinct, all from splitmix_bytes"""
    b = splitmix_bytes(32 + 32 + 32 + 64 + 16, seed * 100003 + i)
    c = {"csec": b[0:32], "ceph": b[32:64], "seph": b[64:96], "entropy": b[96:160], "vnonce": b[160:176]}
    c["cpub"] = M.public_key(c["csec"])
    c["hello"] = M.client_hello(SERVER_PUB, c["ceph"])
    c["welcome"], c["state"] = M.server_welcome(c["hello"], SERVER_SEC, c["seph"], c["entropy"])
    return c


def initiate_of(c, **kw):
    return M.client_initiate(c["welcome"], c["cpub"], c["csec"], SERVER_PUB, c["ceph"], c["vnonce"], **kw)


def make_acceptor(gpu, conns, **kw):
    return gpu.acceptor.CurveAcceptor(SERVER_SEC, ephemeral_secrets=[c["seph"] for c in conns],
                                      entropy=[c["entropy"] for c in conns], **kw)


def cz_hs_server(gpu, c, **kw):
    return gpu.hs.CurveServerHandshake(SERVER_SEC, ephemeral_secret=c["seph"], entropy=c["entropy"], **kw)


def cz_hs_hello(gpu, c, cmd):
    """(rc, event, reply) a cz_hs server gives for `cmd` as its first command"""
    srv = cz_hs_server(gpu, c)
    rc = srv.processHandshakeCommand(cmd)
    if rc != 0:
        assert rc == gpu.hs.EPROTO
        return gpu.lib.CZ_EPROTO, srv.last_event, b""
    ev = srv.last_event
    r, reply = srv.nextHandshakeCommand()
    assert r == 0
    return gpu.lib.CZ_OK, ev, reply.data


def test_golden_libzmq_session_batch_of_one(gpu):
    s = S["server_session"]
    acc = gpu.acceptor.CurveAcceptor(SERVER_SEC, ephemeral_secrets=[H(s["server_ephemeral_secret"])],
                                     entropy=[H(s["entropy"])], max_pending=1)
    ((rc, ev, slot, welcome),) = acc.hello([H(s["hello"])])
    assert (rc, ev) == (0, 0) and slot == 0 and welcome == H(s["welcome"])
    assert acc.pending() == 1
    ((rc, ev, slot2, ready),) = acc.initiate([slot], [H(s["initiate"])])
    assert (rc, ev, slot2) == (0, 0, slot) and ready == H(s["ready"])
    assert acc.session(slot) == (H(s["precom"]), 2, 2)
    assert acc.client_key(slot) == CLIENT_PUB
    assert acc.peer_property(slot, "Socket-Type") == b"PAIR" and acc.peer_property(slot, "Identity") is None
    # the recorded MESSAGE traffic, through the engine and through a mechanism
    eng = gpu.engine.CurveBatchEngine(arena_bytes=1 << 20)
    c = eng.add_accepted(acc, slot)
    eng.recv(c, b"".join(v2_encode(H(m["body"])) for m in s["c2s"]))
    eng.flush_in()
    assert eng.error(c) == (0, 0)
    assert eng.messages_in(c) == [(splitmix_bytes(m["n"], m["seed"]), m["flags"]) for m in s["c2s"]]
    for m in s["s2c"]:
        eng.send(c, splitmix_bytes(m["n"], m["seed"]), more=bool(m["flags"] & 1))
    eng.flush_out()
    assert eng.wire_out(c) == b"".join(v2_encode(H(m["body"])) for m in s["s2c"])
    from jeromq_amd.mechanism import Msg
    mech = acc.mechanism(slot)
    got = mech.decode(Msg(H(s["c2s"][0]["body"])))
    assert got is not None and got.data == splitmix_bytes(s["c2s"][0]["n"], s["c2s"][0]["seed"])
    acc.release(slot)
    assert acc.pending() == 0
    with pytest.raises(gpu.lib.CzError):
        acc.session(slot)


def test_wave_edges_130_connections(gpu):
    """two full 64-lane workgroups and a 2-lane tail (stage 1 runs 390 key-agreement lanes)"""
    n = 130
    conns = [conn(i, 2) for i in range(n)]
    acc = make_acceptor(gpu, conns, max_pending=n)
    r1 = acc.hello([c["hello"] for c in conns])
    assert [(rc, ev) for rc, ev, _, _ in r1] == [(0, 0)] * n
    slots = [sl for _, _, sl, _ in r1]
    assert sorted(slots) == list(range(n))
    for i, c in enumerate(conns):
        assert r1[i][3] == c["welcome"], f"WELCOME {i}"
    inits = [initiate_of(c) for c in conns]
    r2 = acc.initiate(slots, inits)
    for i, c in enumerate(conns):
        ready, facts = M.server_ready(inits[i], c["state"])
        assert r2[i] == (0, 0, slots[i], ready), f"READY {i}"
        assert acc.session(slots[i]) == (or_beforenm(M.public_key(c["ceph"]), c["seph"]), 2, 2), f"session {i}"
        assert acc.client_key(slots[i]) == c["cpub"]
    # the per-connection state machine with the same injected values: identical bytes
    for i in (0, 63, 64, 127, 128, 129):
        c = conns[i]
        srv = cz_hs_server(gpu, c)
        assert srv.processHandshakeCommand(c["hello"]) == 0
        assert srv.nextHandshakeCommand()[1].data == r1[i][3]
        assert srv.processHandshakeCommand(inits[i]) == 0
        assert srv.nextHandshakeCommand()[1].data == r2[i][3]
        assert srv.session() == acc.session(slots[i]) and srv.client_key() == acc.client_key(slots[i])


def test_every_initiate_length_in_one_batch(gpu):
    """DEALER identities of 0..221 bytes: metadata of 35..256 bytes, INITIATE boxes of 195..416 bytes --
    every Salsa20 block edge and Poly1305 chunk edge the command can reach, partial last chunks included"""
    n = 222
    conns = [conn(i, 3) for i in range(n)]
    ids = [splitmix_bytes(i, 7000 + i) for i in range(n)]
    acc = make_acceptor(gpu, conns, socket_type=ZMQ_ROUTER, max_pending=n)
    r1 = acc.hello([c["hello"] for c in conns])
    assert [r[3] for r in r1] == [c["welcome"] for c in conns]
    slots = [r[2] for r in r1]
    inits = [initiate_of(c, socket_type=ZMQ_DEALER, identity=ids[i]) for i, c in enumerate(conns)]
    assert [len(x) for x in inits] == [113 + 16 + 128 + 35 + i for i in range(n)]
    r2 = acc.initiate(slots, inits)
    for i, c in enumerate(conns):
        ready, facts = M.server_ready(inits[i], c["state"], socket_type=ZMQ_ROUTER)
        assert facts["metadata"] == M.metadata(ZMQ_DEALER, ids[i])
        assert r2[i] == (0, 0, slots[i], ready), f"identity of {i} bytes"
        assert acc.peer_property(slots[i], "Identity") == ids[i], f"identity of {i} bytes"
        assert acc.peer_property(slots[i], "Socket-Type") == b"DEALER"
    with pytest.raises(M.ModelError):     # 257 bytes of metadata: the client refuses to build the command
        initiate_of(conns[0], socket_type=ZMQ_DEALER, identity=bytes(222))


def test_divergent_lanes_in_one_hello_batch(gpu):
    """70 HELLOs, valid ones interleaved with every way a HELLO fails, on both sides of the 64-lane edge.
    Each item must be what a cz_hs server makes of that command.  `HELLP` is among them: Msgs.startsWith
    never looks at a name's last character (the reference's quirk, mirrored), so cz_hs accepts it."""
    n = 70
    conns = [conn(i, 4) for i in range(n)]
    cmds = [c["hello"] for c in conns]

    def flip(b, pos):
        return b[:pos] + bytes([b[pos] ^ 1]) + b[pos + 1:]

    bad = {
        3: cmds[3][:199],                                   # size 199
        10: cmds[10] + b"\x00",                             # size 201
        17: cmds[17][:7] + b"\x01" + cmds[17][8:],          # version 1.1
        24: b"\x05HELLP" + cmds[24][6:],                    # last character of the name
        25: b"\x05HELPO" + cmds[25][6:],                    # a wrong name
        31: flip(cmds[31], 160),                            # the box
        38: flip(cmds[38], 125),                            # the tag
        45: flip(cmds[45], 90),                             # C'
        63: flip(cmds[63], 199),                            # last lane of the first workgroup
        64: flip(cmds[64], 80),                             # first lane of the second
        69: cmds[69][:6] + b"\x02" + cmds[69][7:],          # version 2.0, the last item
    }
    for i, b in bad.items():
        cmds[i] = b
    acc = make_acceptor(gpu, conns, max_pending=n)
    got = acc.hello(cmds)
    for i, c in enumerate(conns):
        rc, ev, slot, reply = got[i]
        if i in bad:
            assert (rc, ev, reply) == cz_hs_hello(gpu, c, cmds[i]), f"item {i}"
            assert (slot >= 0) == (reply[:8] == b"\x07WELCOME")
        else:
            assert (rc, ev, reply) == (0, 0, c["welcome"]) and slot >= 0, f"valid neighbour {i}"
    assert got[3][:2] == got[10][:2] == got[17][:2] == got[69][:2] == (gpu.lib.CZ_EPROTO, MALFORMED_HELLO)
    assert got[25][:2] == (gpu.lib.CZ_EPROTO, UNEXPECTED)
    for i in (31, 38, 45, 63, 64):
        assert got[i] == (0, CRYPTOGRAPHIC, -1, M.ERROR_EMPTY)
    assert got[24][3] == conns[24]["welcome"]
    assert acc.pending() == n - (len(bad) - 1)


def test_stage2_failures_in_one_batch(gpu):
    """SUB clients to a PUB acceptor; every way an INITIATE fails between valid neighbours"""
    L = gpu.lib
    n = 16
    conns = [conn(i, 5) for i in range(n)]
    acc = make_acceptor(gpu, conns, socket_type=ZMQ_PUB, max_pending=n)
    r1 = acc.hello([c["hello"] for c in conns])
    assert [r[3] for r in r1] == [c["welcome"] for c in conns]
    slots = [r[2] for r in r1]
    inits = [initiate_of(c, socket_type=ZMQ_SUB) for c in conns]
    good = list(inits)

    def flip(b, pos):
        return b[:pos] + bytes([b[pos] ^ 1]) + b[pos + 1:]

    other = M.public_key(bytes(range(2, 34)))
    cases = {
        1: (flip(good[1], 60), L.CZ_EPROTO, CRYPTOGRAPHIC),                    # the cookie box
        2: (flip(good[2], 12), L.CZ_EPROTO, CRYPTOGRAPHIC),                    # the cookie nonce
        3: (flip(good[3], 200), L.CZ_EPROTO, CRYPTOGRAPHIC),                   # the INITIATE box
        4: (initiate_of(conns[4], socket_type=ZMQ_SUB, vouch_flip=40), L.CZ_EPROTO, CRYPTOGRAPHIC),   # the vouch
        5: (good[5][:9] + good[0][9:105] + good[5][105:], L.CZ_EPROTO, CRYPTOGRAPHIC),   # connection 0's cookie
        6: (initiate_of(conns[6], socket_type=ZMQ_SUB, vouch_eph_public=other), L.CZ_EPROTO, KEY_EXCHANGE),
        7: (good[7][:256], L.CZ_EPROTO, MALFORMED_INITIATE),                   # size 256
        8: (good[8] + bytes(113 + 144 + 256 + 1 - len(good[8])), L.CZ_EPROTO, MALFORMED_INITIATE),   # box over by one
        9: (initiate_of(conns[9], socket_type=ZMQ_PUB), L.CZ_EINVAL, 0),        # PUB to PUB
        10: (initiate_of(conns[10], meta=M.metadata(ZMQ_SUB)[:-1]), L.CZ_EPROTO, 0),   # truncated metadata
        12: (flip(good[12], 3), L.CZ_EPROTO, UNEXPECTED),                      # not an INITIATE
    }
    assert len(cases[8][0]) == 514 and len(good[3]) > 200
    for i, (cmd, _, _) in cases.items():
        inits[i] = cmd
    r2 = acc.initiate(slots, inits)
    for i, c in enumerate(conns):
        if i in cases:
            assert r2[i] == (cases[i][1], cases[i][2], slots[i], b""), f"case {i}"
            with pytest.raises(L.CzError):
                acc.session(slots[i])
        else:
            ready, facts = M.server_ready(inits[i], c["state"], socket_type=ZMQ_PUB)
            assert r2[i] == (0, 0, slots[i], ready), f"valid neighbour {i}"
            assert acc.session(slots[i]) == (facts["precom"], 2, 2)
            assert acc.peer_property(slots[i], "Socket-Type") == b"SUB"
    # the truncated metadata as cz_hs sees it
    srv = cz_hs_server(gpu, conns[10], socket_type=ZMQ_PUB)
    assert srv.processHandshakeCommand(conns[10]["hello"]) == 0 and srv.nextHandshakeCommand()[0] == 0
    assert srv.processHandshakeCommand(inits[10]) == gpu.hs.EPROTO and srv.last_event == 0
    # the boxes opened where only the metadata failed: the client's key is known; failed slots stay allocated
    assert acc.client_key(slots[9]) == conns[9]["cpub"] and acc.client_key(slots[10]) == conns[10]["cpub"]
    assert acc.pending() == n
    # the good INITIATE after the bad one: the slot has left EXPECT_INITIATE
    again = acc.initiate([slots[1], slots[0]], [good[1], good[0]])
    assert [(rc, ev, reply) for rc, ev, _, reply in again] == [(L.CZ_EINVAL, 0, b"")] * 2


def test_slot_life_cycle(gpu):
    L = gpu.lib
    conns = [conn(i, 6) for i in range(8)]
    acc = make_acceptor(gpu, conns, max_pending=4)
    r1 = acc.hello([c["hello"] for c in conns[:6]])
    assert [r[0] for r in r1] == [0, 0, 0, 0, L.CZ_EAGAIN, L.CZ_EAGAIN]
    assert [r[2] for r in r1[4:]] == [-1, -1] and [r[3] for r in r1[4:]] == [b"", b""]
    assert [r[3] for r in r1[:4]] == [c["welcome"] for c in conns[:4]] and acc.pending() == 4
    slots = [r[2] for r in r1[:4]]
    inits = [initiate_of(c) for c in conns]
    # one batch: a good slot, the same slot again, slot -1, a slot past the table
    r2 = acc.initiate([slots[0], slots[0], -1, 4, 1 << 30], [inits[0]] * 5)
    assert r2[0][0] == 0 and r2[0][3] == M.server_ready(inits[0], conns[0]["state"])[0]
    assert [r[0] for r in r2[1:]] == [L.CZ_EINVAL] * 4 and all(r[3] == b"" for r in r2[1:])
    assert acc.initiate([slots[0]], [inits[0]])[0][0] == L.CZ_EINVAL
    # release: the slot is free, its session is gone, a second release is refused
    first = acc.session(slots[0])
    acc.release(slots[0])
    assert acc.pending() == 3
    with pytest.raises(L.CzError):
        acc.release(slots[0])
    with pytest.raises(L.CzError):
        acc.session(slots[0])
    assert acc.initiate([slots[0]], [inits[0]])[0][0] == L.CZ_EINVAL
    # (the acceptor has seen 6 HELLOs: the next one draws the injected values of index 6)
    ((rc, ev, s6, w6),) = acc.hello([conns[6]["hello"]])
    assert (rc, ev, s6, w6) == (0, 0, slots[0], conns[6]["welcome"]) and acc.pending() == 4
    # the old connection's INITIATE on the reused slot fails; the new one's gives the new session
    assert acc.initiate([s6], [inits[0]])[0][:2] == (L.CZ_EPROTO, CRYPTOGRAPHIC)
    acc.release(s6)
    ((rc, ev, s7, w7),) = acc.hello([conns[7]["hello"]])
    assert (rc, s7, w7) == (0, slots[0], conns[7]["welcome"])
    ((rc, ev, _, ready),) = acc.initiate([s7], [inits[7]])
    assert (rc, ev) == (0, 0) and ready == M.server_ready(inits[7], conns[7]["state"])[0]
    assert acc.session(s7) == (conns[7]["state"]["precom"], 2, 2) and acc.session(s7) != first
    # the untouched neighbours still complete
    r3 = acc.initiate(slots[1:], inits[1:4])
    assert [r[3] for r in r3] == [M.server_ready(inits[i], conns[i]["state"])[0] for i in (1, 2, 3)]
    for s in slots[1:] + [s7]:
        acc.release(s)
    assert acc.pending() == 0


def test_argument_validation(gpu):
    L = gpu.lib
    lib = L.lib()
    c = conn(0, 7)
    acc = make_acceptor(gpu, [c], max_pending=2)
    res = (L.cz_accept_result * 2)()
    reply = ctypes.create_string_buffer(b"\xaa" * 1024, 1024)
    ctypes.memset(res, 0xaa, ctypes.sizeof(res))
    cmd = c["hello"]
    off = np.array([0], dtype=np.uint64)
    size = np.array([200], dtype=np.uint32)
    slot = np.array([0], dtype=np.int32)
    far = np.array([1 << 63], dtype=np.uint64)

    def hello(a=acc._h, count=1, cmds=cmd, nbytes=200, off=off.ctypes.data, size=size.ctypes.data, reply=reply,
              stride=168, res=res):
        return lib.cz_acceptor_hello(a, count, cmds, nbytes, off, size, reply, stride, res, None, None)

    def initiate(a=acc._h, count=1, slot=slot.ctypes.data, cmds=cmd, nbytes=200, off=off.ctypes.data,
                 size=size.ctypes.data, reply=reply, stride=288, res=res):
        return lib.cz_acceptor_initiate(a, count, slot, cmds, nbytes, off, size, reply, stride, res)

    for call in (hello, initiate):
        assert call(count=0) == L.CZ_OK
        assert call(nbytes=199) == L.CZ_EINVAL                    # off + size past cmds_bytes
        assert call(off=far.ctypes.data) == L.CZ_EINVAL
        for null in ("a", "cmds", "off", "size", "reply", "res"):
            assert call(**{null: None}) == L.CZ_EINVAL, null
    assert hello(stride=167) == L.CZ_EINVAL
    assert initiate(stride=287) == L.CZ_EINVAL and initiate(slot=None) == L.CZ_EINVAL
    assert reply.raw == b"\xaa" * 1024 and bytes(res) == b"\xaa" * ctypes.sizeof(res)   # nothing written
    assert acc.pending() == 0
    # and the same call with good arguments goes through
    assert hello() == L.CZ_OK and res[0].rc == 0 and res[0].reply_len == 168 and acc.pending() == 1


def test_product_clients_against_the_acceptor(gpu):
    """fresh keys and production entropy on both sides: 8 CurveClientHandshake objects against one acceptor"""
    n = 8
    hs = gpu.hs
    csecs = [os.urandom(32) for _ in range(n)]
    cpubs = [M.public_key(k) for k in csecs]
    clients = [hs.CurveClientHandshake(cpubs[i], csecs[i], SERVER_PUB, socket_type=ZMQ_DEALER,
                                       identity=b"peer-%d" % i) for i in range(n)]
    acc = gpu.acceptor.CurveAcceptor(SERVER_SEC, socket_type=ZMQ_ROUTER, max_pending=n)
    hellos = [cl.nextHandshakeCommand()[1].data for cl in clients]
    r1 = acc.hello(hellos)
    assert [(r[0], r[1]) for r in r1] == [(0, 0)] * n
    welcomes = [r[3] for r in r1]
    assert len(set(welcomes)) == n and len({w[8:24] for w in welcomes}) == n     # per-connection draws
    for cl, w in zip(clients, welcomes):
        assert cl.processHandshakeCommand(w) == 0
    inits = [cl.nextHandshakeCommand()[1].data for cl in clients]
    slots = [r[2] for r in r1]
    r2 = acc.initiate(slots, inits)
    assert [(r[0], r[1]) for r in r2] == [(0, 0)] * n
    cli_eng = gpu.engine.CurveBatchEngine(arena_bytes=1 << 20)
    srv_eng = gpu.engine.CurveBatchEngine(arena_bytes=1 << 20)
    cc, sc = [], []
    for i, cl in enumerate(clients):
        assert cl.processHandshakeCommand(r2[i][3]) == 0 and cl.status() == hs.Status.READY
        assert cl.peer_property("Socket-Type") == b"ROUTER"
        assert acc.client_key(slots[i]) == cpubs[i] and acc.peer_property(slots[i], "Identity") == b"peer-%d" % i
        assert acc.session(slots[i])[0] == cl.session()[0]
        cc.append(cli_eng.add_session(cl))
        sc.append(srv_eng.add_accepted(acc, slots[i]))
        acc.release(slots[i])
    assert acc.pending() == 0
    msgs = [splitmix_bytes(10 + 37 * i, 4242 + i) for i in range(n)]
    for src, sconn, dst, dconn in ((cli_eng, cc, srv_eng, sc), (srv_eng, sc, cli_eng, cc)):
        for i in range(n):
            src.send(sconn[i], msgs[i])
            src.send(sconn[i], msgs[i][::-1], more=True)
        src.flush_out()
        for i in range(n):
            dst.recv(dconn[i], src.wire_out(sconn[i]))
        dst.flush_in()
        for i in range(n):
            assert dst.error(dconn[i]) == (0, 0)
            assert dst.messages_in(dconn[i]) == [(msgs[i], 0), (msgs[i][::-1], 1)]
