"""GPU: the batched CURVE client handshake (jeromq_amd.connector, cz_connector.cpp, cz_connect_kernels.h).

Yardsticks: the libzmq 4.3.4 client session of tests/golden/libzmq_session.json, the CPU model of
tests/hs_model.py (anchored to libzmq by tests/test_hs_model.py) and, where the question is what the
per-connection state machine does with a command, a CurveClientHandshake (cz_hs) fed the same bytes.
The connector is never checked against itself.  Shapes are the smallest at which the
lane-per-connection kernels can go wrong: one lane, two full 64-lane workgroups plus a tail, the
INITIATE lengths at chunk and keystream-block edges, every READY length, and batches whose lanes
take different paths."""
import ctypes
import functools
import json
import os
import struct

import numpy as np
import pytest

import hs_model as M
from cz_testlib import splitmix_bytes, v2_encode

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
S = json.load(open(os.path.join(HERE, "golden", "libzmq_session.json")))
CLIENT_PUB = bytes.fromhex("BB88471D65E2659B30C55A5321CEBB5AAB2B70A398645C26DCA2B2FCB43FC518")
CLIENT_SEC = bytes.fromhex("7BB864B489AFA3671FBE69101F94B38972F24816DFB01B51656B3FEC8DFD0888")
SERVER_PUB = bytes.fromhex("54FCBA24E93249969316FB617C872BB0C1D1FF14800427C594CBFACF1BC2D652")
SERVER_SEC = bytes.fromhex("8E0BDD697628B91D8F245587EE95C5B04D48963F79259877B49CD9063AEAD3B7")

UNEXPECTED, MALFORMED_ERROR, MALFORMED_READY = 0x10000001, 0x10000015, 0x10000016
CRYPTOGRAPHIC, ZAP_MALFORMED_REPLY = 0x11000001, 0x20000001
ZMQ_PAIR, ZMQ_PUB, ZMQ_SUB, ZMQ_DEALER, ZMQ_ROUTER = 0, 1, 2, 5, 6


def H(x):
    return bytes.fromhex(x)


def flip(b, pos):
    return b[:pos] + bytes([b[pos] ^ 1]) + b[pos + 1:]


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from jeromq_amd import _lib, acceptor, connector, engine, handshake
    return type("G", (), {"lib": _lib, "acceptor": acceptor, "connector": connector, "engine": engine,
                          "hs": handshake})


@functools.lru_cache(maxsize=None)
def servers():
    """three servers a batch can dial: the published test key and two more"""
    out = [(SERVER_SEC, SERVER_PUB)]
    for seed in (555001, 555002):
        sec = splitmix_bytes(32, seed)
        out.append((sec, M.public_key(sec)))
    return out


@functools.lru_cache(maxsize=None)
def conn(i, seed, srv=0, ctype=ZMQ_PAIR, cident=b"", stype=ZMQ_PAIR, sident=b"", ready_nonce=1, vnonce=None):
    """connection i of a test, wholly from the CPU model: the client's short-term secret and vouch nonce,
    the server's short-term secret and entropy (all distinct, all from splitmix_bytes), and the four
    commands an honest pair exchanges.  The client's long-term pair is CLIENT_PUB / CLIENT_SEC."""
    b = splitmix_bytes(32 + 32 + 64 + 16, seed * 100003 + i)
    c = {"ceph": b[0:32], "seph": b[32:64], "entropy": b[64:128], "vnonce": vnonce or b[128:144]}
    ssec, c["spub"] = servers()[srv]
    c["hello"] = M.client_hello(c["spub"], c["ceph"])
    c["welcome"], c["state"] = M.server_welcome(c["hello"], ssec, c["seph"], c["entropy"])
    c["initiate"] = M.client_initiate(c["welcome"], CLIENT_PUB, CLIENT_SEC, c["spub"], c["ceph"], c["vnonce"],
                                      socket_type=ctype, identity=cident)
    got = M.server_ready(c["initiate"], c["state"], socket_type=stype, identity=sident, nonce=ready_nonce)
    assert not isinstance(got, str), f"the model server refuses the model client's INITIATE: {got}"
    c["ready"], facts = got
    assert facts["client_key"] == CLIENT_PUB
    c["precom"] = c["state"]["precom"]
    return c


def make_connector(gpu, conns, **kw):
    """vouch nonces are drawn per command given to welcome(): connection i % len(conns) for the i-th"""
    return gpu.connector.CurveConnector(CLIENT_PUB, CLIENT_SEC, ephemeral_secrets=[c["ceph"] for c in conns],
                                        vouch_nonces=lambda i: conns[i % len(conns)]["vnonce"], **kw)


def cz_hs_client(gpu, c, upto, **kw):
    """a cz_hs client with connection c's injected values, moved to EXPECT_WELCOME ("welcome") or
    EXPECT_READY ("ready") by the model's commands"""
    cli = gpu.hs.CurveClientHandshake(CLIENT_PUB, CLIENT_SEC, c["spub"], ephemeral_secret=c["ceph"],
                                      entropy=c["vnonce"], **kw)
    rc, hello = cli.nextHandshakeCommand()
    assert rc == 0 and hello.data == c["hello"]
    if upto == "ready":
        assert cli.processHandshakeCommand(c["welcome"]) == 0
        rc, init = cli.nextHandshakeCommand()
        assert rc == 0 and init.data == c["initiate"]
    return cli


def cz_hs_verdict(gpu, cli, cmd):
    """(rc, event, error status) of a cz_hs client for `cmd`, in the connector's terms"""
    rc = cli.processHandshakeCommand(cmd)
    rc = {0: gpu.lib.CZ_OK, gpu.hs.EPROTO: gpu.lib.CZ_EPROTO, gpu.hs.EINVAL: gpu.lib.CZ_EINVAL}[rc]
    return rc, cli.last_event, gpu.lib.lib().cz_hs_error_status(cli._h)


def handshake(con, conns):
    """all three stages for honest peers; returns the slots"""
    r1 = con.hello([c["spub"] for c in conns])
    assert [(r[0], r[1], r[3]) for r in r1] == [(0, 0, c["hello"]) for c in conns]
    slots = [r[2] for r in r1]
    r2 = con.welcome(slots, [c["welcome"] for c in conns])
    assert r2 == [(0, 0, s, c["initiate"]) for s, c in zip(slots, conns)]
    r3 = con.ready(slots, [c["ready"] for c in conns])
    assert r3 == [(0, 0, s, b"") for s in slots]
    return slots


def test_golden_libzmq_session_batch_of_one(gpu):
    g = S["client_handshake"]
    con = gpu.connector.CurveConnector(CLIENT_PUB, CLIENT_SEC, ephemeral_secrets=[H(S["client_ephemeral_secret"])],
                                       vouch_nonces=[H(g["vouch_nonce"])], max_pending=1)
    ((rc, ev, slot, hello),) = con.hello([SERVER_PUB])
    assert (rc, ev, slot) == (0, 0, 0) and hello == H(g["hello"])
    assert con.pending() == 1 and con.server_key(slot) == SERVER_PUB
    ((rc, ev, slot2, initiate),) = con.welcome([slot], [H(g["welcome"])])
    assert (rc, ev, slot2) == (0, 0, slot) and initiate == H(g["initiate"])
    assert con.ready([slot], [H(g["ready"])]) == [(0, 0, slot, b"")]
    # the per-connection state machine on the same commands
    cli = gpu.hs.CurveClientHandshake(CLIENT_PUB, CLIENT_SEC, SERVER_PUB,
                                      ephemeral_secret=H(S["client_ephemeral_secret"]), entropy=H(g["vouch_nonce"]))
    assert cli.nextHandshakeCommand()[1].data == hello and cli.processHandshakeCommand(H(g["welcome"])) == 0
    assert cli.nextHandshakeCommand()[1].data == initiate and cli.processHandshakeCommand(H(g["ready"])) == 0
    assert con.session(slot) == cli.session() == (H(S["precom"]), 3, S["ready_nonce"])
    assert con.peer_property(slot, "Socket-Type") == b"PAIR" and con.peer_property(slot, "Identity") is None
    assert con.error_status(slot) == 0
    # the recorded MESSAGE traffic, through the engine and through a mechanism
    eng = gpu.engine.CurveBatchEngine(arena_bytes=1 << 20)
    c = eng.add_connected(con, slot)
    eng.recv(c, H(S["s2c_wire"]))
    eng.flush_in()
    assert eng.error(c) == (0, 0)
    assert eng.messages_in(c) == [(splitmix_bytes(m["n"], m["seed"]), m["flags"]) for m in S["s2c"]]
    for m in S["c2s"]:
        eng.send(c, splitmix_bytes(m["n"], m["seed"]), more=bool(m["flags"] & 1))
    eng.flush_out()
    assert eng.wire_out(c) == b"".join(v2_encode(H(m["body"])) for m in S["c2s"])
    from jeromq_amd.mechanism import Msg
    mech = con.mechanism(slot)
    for m in S["c2s"]:
        assert mech.encode(Msg(splitmix_bytes(m["n"], m["seed"]), m["flags"])).data.hex() == m["body"]
    for m in S["s2c"]:
        got = mech.decode(Msg(H(m["body"])))
        assert got is not None and got.data == splitmix_bytes(m["n"], m["seed"])
    con.release(slot)
    assert con.pending() == 0
    with pytest.raises(gpu.lib.CzError):
        con.session(slot)


def test_wave_edges_130_connections_three_servers(gpu):
    """two full 64-lane workgroups and a 2-lane tail (260 key-agreement lanes per stage), three server
    keys mixed in one batch"""
    n = 130
    conns = [conn(i, 12, srv=(i * 7) % 3) for i in range(n)]
    assert len({c["spub"] for c in conns}) == 3
    con = make_connector(gpu, conns, max_pending=n)
    r1 = con.hello([c["spub"] for c in conns])
    assert [(rc, ev) for rc, ev, _, _ in r1] == [(0, 0)] * n
    slots = [r[2] for r in r1]
    assert sorted(slots) == list(range(n))
    for i, c in enumerate(conns):
        assert r1[i][3] == c["hello"], f"HELLO {i}"
        assert con.server_key(slots[i]) == c["spub"]
    r2 = con.welcome(slots, [c["welcome"] for c in conns])
    for i, c in enumerate(conns):
        # (conn() has had the model server accept this very INITIATE)
        assert r2[i] == (0, 0, slots[i], c["initiate"]), f"INITIATE {i}"
    r3 = con.ready(slots, [c["ready"] for c in conns])
    for i, c in enumerate(conns):
        assert r3[i] == (0, 0, slots[i], b""), f"READY {i}"
        assert con.session(slots[i]) == (c["precom"], 3, 1), f"session {i}"
    # the per-connection state machine with the same injected values: the same session
    for i in (0, 63, 64, 129):
        cli = cz_hs_client(gpu, conns[i], "ready")
        assert cli.processHandshakeCommand(conns[i]["ready"]) == 0
        assert cli.session() == con.session(slots[i])


def test_initiate_lengths_at_chunk_and_block_edges(gpu):
    """DEALER identities of 0, 12, 14, 60, 61, 62 and 221 bytes: the INITIATE box plaintext is 163 + identity
    bytes and sits 32 bytes into the XSalsa20 stream"""
    lens = [0, 12, 14, 60, 61, 62, 221]
    plain = [128 + len(M.metadata(ZMQ_DEALER, bytes(k))) for k in lens]
    assert plain == [163 + k for k in lens]
    assert plain[1] % 16 == 15 and plain[2] % 16 == 1                    # last Poly1305 chunk of 15 bytes, of 1 byte
    assert [(32 + p) % 64 for p in plain[3:6]] == [63, 0, 1]              # around a 64-byte keystream block edge
    assert plain[6] - 128 == 256                                         # the metadata cap
    for k in lens:
        ident = splitmix_bytes(k, 8100 + k)
        c = conn(k, 13, ctype=ZMQ_DEALER, cident=ident, stype=ZMQ_ROUTER)
        con = make_connector(gpu, [c], socket_type=ZMQ_DEALER, identity=ident, max_pending=1)
        ((rc, ev, slot, hello),) = con.hello([c["spub"]])
        assert (rc, ev, hello) == (0, 0, c["hello"])
        ((rc, ev, _, init),) = con.welcome([slot], [c["welcome"]])
        assert (rc, ev) == (0, 0) and len(init) == 257 + 35 + k
        assert init == c["initiate"], f"identity of {k} bytes"
        assert con.ready([slot], [c["ready"]]) == [(0, 0, slot, b"")]
        assert con.session(slot) == (c["precom"], 3, 1) and con.peer_property(slot, "Socket-Type") == b"ROUTER"
        con.close()
    with pytest.raises(gpu.lib.CzError):   # 257 bytes of metadata
        gpu.connector.CurveConnector(CLIENT_PUB, CLIENT_SEC, socket_type=ZMQ_DEALER, identity=bytes(222))


def test_every_ready_length_in_one_batch(gpu):
    """ROUTER servers with identities of 0..221 bytes: READY plaintexts of 35..256 bytes, every Salsa20 block
    edge and Poly1305 chunk edge the command can reach, partial last chunks included"""
    n = 222
    ids = [splitmix_bytes(i, 9000 + i) for i in range(n)]
    conns = [conn(i, 14, ctype=ZMQ_DEALER, stype=ZMQ_ROUTER, sident=ids[i]) for i in range(n)]
    assert [len(c["ready"]) for c in conns] == [14 + 16 + 35 + i for i in range(n)]
    con = make_connector(gpu, conns, socket_type=ZMQ_DEALER, max_pending=n)
    slots = handshake(con, conns)
    for i, c in enumerate(conns):
        assert con.peer_property(slots[i], "Identity") == ids[i], f"identity of {i} bytes"
        assert con.peer_property(slots[i], "Socket-Type") == b"ROUTER"
        assert con.session(slots[i]) == (c["precom"], 3, 1)


def test_divergent_lanes_in_one_welcome_batch(gpu):
    """valid WELCOMEs interleaved with every way stage 2 can go: each item must be what a cz_hs client
    waiting for its WELCOME makes of that command"""
    L = gpu.lib
    n = 20
    conns = [conn(i, 15) for i in range(n)]
    con = make_connector(gpu, conns, max_pending=n)
    r1 = con.hello([c["spub"] for c in conns])
    assert [r[3] for r in r1] == [c["hello"] for c in conns]
    slots = [r[2] for r in r1]
    good = [c["welcome"] for c in conns]
    other_sec, other_pub = servers()[1]
    c7 = conns[7]
    under_other_key = M.server_welcome(M.client_hello(other_pub, c7["ceph"]), other_sec, c7["seph"], c7["entropy"])[0]
    assert len(under_other_key) == 168 and under_other_key[:8] == b"\x07WELCOME"
    bad = {
        1: (good[1][:167], L.CZ_EPROTO, MALFORMED_READY, 0),                  # sic: the reference's event
        2: (good[2] + b"\x00", L.CZ_EPROTO, MALFORMED_READY, 0),
        3: (flip(good[3], 24 + 3), L.CZ_EPROTO, CRYPTOGRAPHIC, 0),             # the tag
        4: (flip(good[4], 100), L.CZ_EPROTO, CRYPTOGRAPHIC, 0),                # the box body
        5: (good[6], L.CZ_EPROTO, CRYPTOGRAPHIC, 0),                           # connection 6's WELCOME
        7: (under_other_key, L.CZ_EPROTO, CRYPTOGRAPHIC, 0),
        8: (conns[8]["ready"], L.CZ_EPROTO, UNEXPECTED, 0),
        9: (b"\x08INITIATE" + bytes(100), L.CZ_EPROTO, UNEXPECTED, 0),
        10: (b"\x05ERROR\x00", L.CZ_OK, 0, 0),
        11: (b"\x05ERROR\x03400", L.CZ_OK, 0, 400),
        13: (b"\x05ERROR\x09ab", L.CZ_EPROTO, MALFORMED_ERROR, 0),             # the reason overruns the command
        14: (b"\x05ERROR\x03abc", L.CZ_EPROTO, ZAP_MALFORMED_REPLY, 0),
        19: (flip(good[19], 167), L.CZ_EPROTO, CRYPTOGRAPHIC, 0),              # the last byte of the last item
    }
    cmds = list(good)
    for i, (cmd, _, _, _) in bad.items():
        cmds[i] = cmd
    r2 = con.welcome(slots, cmds)
    for i, c in enumerate(conns):
        if i in bad:
            verdict = cz_hs_verdict(gpu, cz_hs_client(gpu, c, "welcome"), cmds[i])
            assert (r2[i][0], r2[i][1], con.error_status(slots[i])) == verdict == bad[i][1:], f"item {i}"
            assert r2[i][2:] == (slots[i], b"")
        else:
            assert r2[i] == (0, 0, slots[i], c["initiate"]), f"valid neighbour {i}"
    assert con.pending() == n
    # a valid WELCOME after the rejected command, the ERROR included: the slot takes no further command
    failed = sorted(bad)
    again = con.welcome([slots[i] for i in failed], [good[i] for i in failed])
    assert again == [(L.CZ_EINVAL, 0, -1, b"")] * len(failed)
    # the good lanes complete
    ok = [i for i in range(n) if i not in bad]
    assert con.ready([slots[i] for i in ok], [conns[i]["ready"] for i in ok]) == [(0, 0, slots[i], b"") for i in ok]
    assert [con.session(slots[i])[0] for i in ok] == [conns[i]["precom"] for i in ok]


def test_divergent_lanes_in_one_ready_batch(gpu):
    """the same for stage 3, against a cz_hs client waiting for its READY"""
    L = gpu.lib
    n = 12
    big = (1 << 32) + 5
    conns = [conn(i, 16, ready_nonce=big if i == 4 else 1) for i in range(n)]
    con = make_connector(gpu, conns, max_pending=n)
    r1 = con.hello([c["spub"] for c in conns])
    slots = [r[2] for r in r1]
    assert con.welcome(slots, [c["welcome"] for c in conns]) == [(0, 0, s, c["initiate"]) for s, c in zip(slots, conns)]
    good = [c["ready"] for c in conns]
    n8 = struct.pack(">Q", 1)

    def ready_with(c, meta):
        return b"\x05READY" + n8 + M._seal(meta, b"CurveZMQREADY---" + n8, c["precom"])

    cases = {
        1: (good[1][:29], L.CZ_EPROTO, MALFORMED_READY, 0),
        2: (good[2] + bytes(287 - len(good[2])), L.CZ_EPROTO, MALFORMED_READY, 0),     # a box of 16 + 16 + 257 bytes
        3: (flip(good[3], 14 + 2), L.CZ_EPROTO, CRYPTOGRAPHIC, 0),                     # the tag
        4: (good[4], L.CZ_OK, 0, 0),                                                   # sealed under nonce 2^32 + 5
        5: (ready_with(conns[5], M.metadata(ZMQ_PUB)), L.CZ_EINVAL, 0, 0),             # PUB answers a PAIR
        6: (ready_with(conns[6], M.metadata(ZMQ_PAIR)[:-1]), L.CZ_EPROTO, 0, 0),       # truncated metadata
        8: (conns[8]["welcome"], L.CZ_EPROTO, UNEXPECTED, 0),
        9: (b"\x05ERROR\x03500", L.CZ_OK, 0, 500),
        11: (flip(good[11], len(good[11]) - 1), L.CZ_EPROTO, CRYPTOGRAPHIC, 0),        # the last byte of the last item
    }
    assert len(cases[2][0]) == 287 and good[4][6:14] == struct.pack(">Q", big)
    cmds = list(good)
    for i, (cmd, _, _, _) in cases.items():
        cmds[i] = cmd
    r3 = con.ready(slots, cmds)
    for i, c in enumerate(conns):
        if i in cases:
            cli = cz_hs_client(gpu, c, "ready")
            verdict = cz_hs_verdict(gpu, cli, cmds[i])
            assert (r3[i][0], r3[i][1], con.error_status(slots[i])) == verdict == cases[i][1:], f"item {i}"
            assert r3[i][2:] == (slots[i], b"")
            if i == 4:
                assert con.session(slots[i]) == cli.session() == (c["precom"], 3, big)
            else:
                with pytest.raises(L.CzError):
                    con.session(slots[i])
        else:
            assert r3[i] == (0, 0, slots[i], b"") and con.session(slots[i]) == (c["precom"], 3, 1), f"neighbour {i}"
    # the good READY after the bad one: the slot has left EXPECT_READY; so has a connected one
    again = con.ready(slots, good)
    assert again == [(L.CZ_EINVAL, 0, -1, b"")] * n
    assert con.pending() == n


def test_slot_life_cycle(gpu):
    L = gpu.lib
    vn = splitmix_bytes(16, 1717)   # one vouch nonce for all: welcome() draws them by command, not by slot
    conns = [conn(i, 17, vnonce=vn) for i in range(8)]
    con = make_connector(gpu, conns, max_pending=4)
    r1 = con.hello([c["spub"] for c in conns[:6]])
    assert [r[0] for r in r1] == [0, 0, 0, 0, L.CZ_EAGAIN, L.CZ_EAGAIN]
    assert [r[2:] for r in r1[4:]] == [(-1, b"")] * 2
    assert [r[3] for r in r1[:4]] == [c["hello"] for c in conns[:4]] and con.pending() == 4
    slots = [r[2] for r in r1[:4]]
    refused = (L.CZ_EINVAL, 0, -1, b"")
    # a stage on a slot in the wrong state: refused, and the slot stays where it was
    assert con.ready([slots[0]], [conns[0]["ready"]]) == [refused]
    # one batch: a good slot, the same slot again (the first item takes it), slot -1, slots past the table
    w0 = conns[0]["welcome"]
    r2 = con.welcome([slots[0], slots[0], -1, 4, 1 << 30], [w0] * 5)
    assert r2 == [(0, 0, slots[0], conns[0]["initiate"])] + [refused] * 4
    assert con.welcome([slots[0]], [w0]) == [refused]      # it waits for its READY now
    assert con.ready([slots[0], slots[0]], [conns[0]["ready"]] * 2) == [(0, 0, slots[0], b""), refused]
    # release: the slot is free, its session is gone, a second release is refused
    first = con.session(slots[0])
    assert first == (conns[0]["precom"], 3, 1)
    con.release(slots[0])
    assert con.pending() == 3
    with pytest.raises(L.CzError):
        con.release(slots[0])
    with pytest.raises(L.CzError):
        con.session(slots[0])
    with pytest.raises(L.CzError):
        con.server_key(slots[0])
    assert con.welcome([slots[0]], [w0]) == [refused] and con.ready([slots[0]], [conns[0]["ready"]]) == [refused]
    # (the connector has dialled 6 connections: the next one draws the injected secret of index 6)
    ((rc, ev, s6, h6),) = con.hello([conns[6]["spub"]])
    assert (rc, ev, s6, h6) == (0, 0, slots[0], conns[6]["hello"]) and con.pending() == 4
    # the old connection's WELCOME on the reused slot does not open; the slot has failed and stays allocated
    assert con.welcome([s6], [w0]) == [(L.CZ_EPROTO, CRYPTOGRAPHIC, s6, b"")]
    assert con.welcome([s6], [conns[6]["welcome"]]) == [refused] and con.pending() == 4
    con.release(s6)
    ((rc, ev, s7, h7),) = con.hello([conns[7]["spub"]])
    assert (rc, s7, h7) == (0, slots[0], conns[7]["hello"])
    assert con.welcome([s7], [conns[7]["welcome"]]) == [(0, 0, s7, conns[7]["initiate"])]
    assert con.ready([s7], [conns[7]["ready"]]) == [(0, 0, s7, b"")]
    assert con.session(s7) == (conns[7]["precom"], 3, 1) and con.session(s7) != first
    # the untouched neighbours still complete
    assert con.welcome(slots[1:], [conns[i]["welcome"] for i in (1, 2, 3)]) == \
        [(0, 0, slots[i], conns[i]["initiate"]) for i in (1, 2, 3)]
    assert con.ready(slots[1:], [conns[i]["ready"] for i in (1, 2, 3)]) == [(0, 0, s, b"") for s in slots[1:]]
    for s in slots[1:] + [s7]:
        con.release(s)
    assert con.pending() == 0


def test_argument_validation(gpu):
    L = gpu.lib
    lib = L.lib()
    c = conn(0, 18)
    con = make_connector(gpu, [c], max_pending=2)
    res = (L.cz_accept_result * 2)()
    reply = ctypes.create_string_buffer(b"\xaa" * 2048, 2048)
    ctypes.memset(res, 0xaa, ctypes.sizeof(res))
    cmd = c["welcome"]
    off = np.array([0], dtype=np.uint64)
    size = np.array([168], dtype=np.uint32)
    slot = np.array([0], dtype=np.int32)
    far = np.array([1 << 63], dtype=np.uint64)

    def hello(a=con._h, count=1, keys=c["spub"], reply=reply, stride=200, res=res):
        return lib.cz_connector_hello(a, count, keys, reply, stride, res, None)

    def welcome(a=con._h, count=1, slot=slot.ctypes.data, cmds=cmd, nbytes=168, off=off.ctypes.data,
                size=size.ctypes.data, reply=reply, stride=513, res=res):
        return lib.cz_connector_welcome(a, count, slot, cmds, nbytes, off, size, reply, stride, res, None)

    def ready(a=con._h, count=1, slot=slot.ctypes.data, cmds=cmd, nbytes=168, off=off.ctypes.data,
              size=size.ctypes.data, res=res):
        return lib.cz_connector_ready(a, count, slot, cmds, nbytes, off, size, res)

    for call in (hello, welcome, ready):
        assert call(count=0) == L.CZ_OK
    for null in ("a", "keys", "reply", "res"):
        assert hello(**{null: None}) == L.CZ_EINVAL, null
    for call, nulls in ((welcome, ("a", "slot", "cmds", "off", "size", "reply", "res")),
                        (ready, ("a", "slot", "cmds", "off", "size", "res"))):
        assert call(nbytes=167) == L.CZ_EINVAL                   # off + size past cmds_bytes
        assert call(off=far.ctypes.data) == L.CZ_EINVAL
        for null in nulls:
            assert call(**{null: None}) == L.CZ_EINVAL, null
    assert hello(stride=199) == L.CZ_EINVAL and welcome(stride=512) == L.CZ_EINVAL
    assert reply.raw == b"\xaa" * 2048 and bytes(res) == b"\xaa" * ctypes.sizeof(res)   # nothing written
    assert con.pending() == 0
    # and the same calls with good arguments go through (production entropy: the HELLO is a fresh one)
    assert hello() == L.CZ_OK and res[0].rc == 0 and res[0].reply_len == 200 and con.pending() == 1
    assert reply.raw[:8] == b"\x05HELLO\x01\x00" and reply.raw[200:] == b"\xaa" * (2048 - 200)
    slot[0] = res[0].slot
    assert welcome() == L.CZ_OK and (res[0].rc, res[0].event & 0xffffffff) == (L.CZ_EPROTO, CRYPTOGRAPHIC)


def test_connector_and_acceptor_on_the_device_with_production_entropy(gpu):
    """130 handshakes between a connector and an acceptor, nothing injected on either side"""
    n = 130
    csec = os.urandom(32)
    cpub = M.public_key(csec)
    con = gpu.connector.CurveConnector(cpub, csec, socket_type=ZMQ_DEALER, identity=b"collector", max_pending=n)
    acc = gpu.acceptor.CurveAcceptor(SERVER_SEC, socket_type=ZMQ_ROUTER, identity=b"front", max_pending=n)
    r1 = con.hello([SERVER_PUB] * n)
    assert [(r[0], r[1]) for r in r1] == [(0, 0)] * n
    cs = [r[2] for r in r1]
    hellos = [r[3] for r in r1]
    assert len({h[80:112] for h in hellos}) == n                      # 130 distinct C'
    a1 = acc.hello(hellos)
    assert [(r[0], r[1]) for r in a1] == [(0, 0)] * n
    ss = [r[2] for r in a1]
    r2 = con.welcome(cs, [r[3] for r in a1])
    assert [(r[0], r[1]) for r in r2] == [(0, 0)] * n
    inits = [r[3] for r in r2]
    assert len({x[113 + 16:113 + 64] for x in inits}) == n            # per-connection vouch nonces -> boxes
    a2 = acc.initiate(ss, inits)
    assert [(r[0], r[1]) for r in a2] == [(0, 0)] * n
    r3 = con.ready(cs, [r[3] for r in a2])
    assert [(r[0], r[1]) for r in r3] == [(0, 0)] * n
    keys = set()
    for i in range(n):
        ck, cn, cpn = con.session(cs[i])
        sk, sn, spn = acc.session(ss[i])
        assert ck == sk, f"connection {i}"
        assert (cn, cpn) == (3, 1) and (sn, spn) == (2, 2)            # as a cz_hs client / server pair
        assert acc.client_key(ss[i]) == cpub
        assert con.peer_property(cs[i], "Identity") == b"front" and acc.peer_property(ss[i], "Identity") == b"collector"
        keys.add(ck)
    assert len(keys) == n
    few = [0, 63, 64, 129]
    cli_eng = gpu.engine.CurveBatchEngine(arena_bytes=1 << 20)
    srv_eng = gpu.engine.CurveBatchEngine(arena_bytes=1 << 20)
    cc = [cli_eng.add_connected(con, cs[i]) for i in few]
    sc = [srv_eng.add_accepted(acc, ss[i]) for i in few]
    for i in range(n):
        con.release(cs[i])
        acc.release(ss[i])
    assert con.pending() == 0 and acc.pending() == 0
    msgs = [splitmix_bytes(10 + 37 * k, 5150 + k) for k in range(len(few))]
    for src, sconn, dst, dconn in ((cli_eng, cc, srv_eng, sc), (srv_eng, sc, cli_eng, cc)):
        for k in range(len(few)):
            src.send(sconn[k], msgs[k])
            src.send(sconn[k], msgs[k][::-1], more=True)
        src.flush_out()
        for k in range(len(few)):
            dst.recv(dconn[k], src.wire_out(sconn[k]))
        dst.flush_in()
        for k in range(len(few)):
            assert dst.error(dconn[k]) == (0, 0)
            assert dst.messages_in(dconn[k]) == [(msgs[k], 0), (msgs[k][::-1], 1)]
