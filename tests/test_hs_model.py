"""CPU: the handshake model of tests/hs_model.py against the recorded libzmq 4.3.4 sessions
(tests/golden/libzmq_session.json).  With the recorded secrets and random draws it must reproduce
what our client sent to libzmq and what our server sent to libzmq's client, byte for byte, and open
what libzmq sent back: that anchors the model to libzmq, not to the code it later judges on the GPU."""
import json
import os

import pytest

import hs_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
S = json.load(open(os.path.join(HERE, "golden", "libzmq_session.json")))
CLIENT_PUB = bytes.fromhex("BB88471D65E2659B30C55A5321CEBB5AAB2B70A398645C26DCA2B2FCB43FC518")
CLIENT_SEC = bytes.fromhex("7BB864B489AFA3671FBE69101F94B38972F24816DFB01B51656B3FEC8DFD0888")
SERVER_PUB = bytes.fromhex("54FCBA24E93249969316FB617C872BB0C1D1FF14800427C594CBFACF1BC2D652")
SERVER_SEC = bytes.fromhex("8E0BDD697628B91D8F245587EE95C5B04D48963F79259877B49CD9063AEAD3B7")


def H(x):
    return bytes.fromhex(x)


def test_keys_are_a_pair():
    assert M.public_key(CLIENT_SEC) == CLIENT_PUB and M.public_key(SERVER_SEC) == SERVER_PUB
    assert M.public_key(H(S["client_ephemeral_secret"])) == H(S["client_ephemeral_public"])


def test_client_side_reproduces_libzmq_session():
    c = S["client_handshake"]
    eph = H(S["client_ephemeral_secret"])
    assert M.client_hello(SERVER_PUB, eph) == H(c["hello"])
    ini = M.client_initiate(H(c["welcome"]), CLIENT_PUB, CLIENT_SEC, SERVER_PUB, eph, H(c["vouch_nonce"]),
                            socket_type=c["socket_type"])
    assert ini == H(c["initiate"])
    srv_eph, _ = M.client_open_welcome(H(c["welcome"]), SERVER_PUB, eph)
    assert srv_eph == H(S["server_ephemeral_public"])
    assert M.client_open_ready(H(c["ready"]), srv_eph, eph) == M.metadata(0)
    assert M.or_beforenm(srv_eph, eph) == H(S["precom"])


def test_server_side_reproduces_libzmq_session():
    s = S["server_session"]
    eph = H(s["server_ephemeral_secret"])
    welcome, state = M.server_welcome(H(s["hello"]), SERVER_SEC, eph, H(s["entropy"]))
    assert welcome == H(s["welcome"])
    assert state["cli_eph"] == H(s["client_ephemeral_public"]) and state["precom"] == H(s["precom"])
    ready, facts = M.server_ready(H(s["initiate"]), state, socket_type=s["socket_type"])
    assert ready == H(s["ready"])
    assert facts["client_key"] == CLIENT_PUB and facts["metadata"] == M.metadata(0)
    assert facts["precom"] == H(s["precom"])


def test_model_failure_paths():
    s = S["server_session"]
    eph = H(s["server_ephemeral_secret"])
    h = bytearray(H(s["hello"]))
    h[150] ^= 1
    assert M.server_welcome(bytes(h), SERVER_SEC, eph, H(s["entropy"])) == (M.ERROR_EMPTY, None)
    assert M.server_welcome(H(s["hello"])[:199], SERVER_SEC, eph, H(s["entropy"])) is None
    _, state = M.server_welcome(H(s["hello"]), SERVER_SEC, eph, H(s["entropy"]))
    for pos, want in ((30, "cryptographic"), (12, "cryptographic"), (200, "cryptographic")):
        i = bytearray(H(s["initiate"]))
        i[pos] ^= 1
        assert M.server_ready(bytes(i), state) == want
    assert M.server_ready(H(s["initiate"])[:256], state) == "malformed"
    assert M.server_ready(H(s["hello"]), state) == "unexpected"


def test_model_client_against_model_server():
    """both halves together, DEALER -> ROUTER with an identity, and the metadata limit"""
    ceph, seph = bytes(range(1, 33)), bytes(range(101, 133))
    ent = bytes(range(64))
    hello = M.client_hello(SERVER_PUB, ceph)
    welcome, state = M.server_welcome(hello, SERVER_SEC, seph, ent)
    ini = M.client_initiate(welcome, CLIENT_PUB, CLIENT_SEC, SERVER_PUB, ceph, bytes(16), socket_type=5,
                            identity=b"peer-7")
    ready, facts = M.server_ready(ini, state, socket_type=6)
    assert facts["client_key"] == CLIENT_PUB and facts["metadata"] == M.metadata(5, b"peer-7")
    assert M.client_open_ready(ready, M.public_key(seph), ceph) == M.metadata(6)
    # a vouch for another C' is a key-exchange failure, not a cryptographic one
    bad = M.client_initiate(welcome, CLIENT_PUB, CLIENT_SEC, SERVER_PUB, ceph, bytes(16),
                            vouch_eph_public=M.public_key(bytes(range(2, 34))))
    assert M.server_ready(bad, state) == "key_exchange"
    # DEALER metadata is 35 + len(identity): 221 bytes of identity is the most an INITIATE carries
    assert len(M.metadata(5, bytes(221))) == 256
    M.client_initiate(welcome, CLIENT_PUB, CLIENT_SEC, SERVER_PUB, ceph, bytes(16), socket_type=5, identity=bytes(221))
    with pytest.raises(M.ModelError):
        M.client_initiate(welcome, CLIENT_PUB, CLIENT_SEC, SERVER_PUB, ceph, bytes(16), socket_type=5,
                          identity=bytes(222))
