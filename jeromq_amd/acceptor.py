"""Batched CURVE server handshake over the C-ABI (cz_acceptor_*): the server half of
CurveServerMechanism's handshake (CurveServerMechanism.java:254-517) for many connections per call.

    acc = CurveAcceptor(server_secret, socket_type=ZMQ_ROUTER, max_pending=1 << 16)
    for (rc, event, slot, welcome), conn in zip(acc.hello(hellos), conns): ...   # N HELLO -> N WELCOME
    for (rc, event, slot, ready), conn in zip(acc.initiate(slots, initiates), conns): ...
    acc.client_key(slot)                       # allow-list check before READY is sent
    c = engine.add_accepted(acc, slot)         # the session moves to the batching engine
    acc.release(slot)
    ids = engine.add_accepted_many(acc, slots); acc.release_many(slots)   # the same for many slots at once

Each stage is a fixed number of device launches and one synchronisation whatever the batch size
(jeromq_amd/csrc/cz_acceptor.cpp).  Every item behaves as one CurveServerHandshake fed the same
command.  ZAP is out of scope.  session, peer_property, release, pending and close: _hs_batch.py.
"""
import ctypes

from ._hs_batch import _HsBatch
from .handshake import ZMQ_PAIR
from .mechanism import CurveServerMechanism

HELLO_REPLY = 168     # the WELCOME command
INITIATE_REPLY = 288  # READY: 14 + 16 + at most 256 bytes of metadata, rounded up


class CurveAcceptor(_HsBatch):
    def __init__(self, secret_key, socket_type=ZMQ_PAIR, identity=b"", max_pending=1024, device=0,
                 ephemeral_secrets=None, entropy=None):
        """ephemeral_secrets / entropy (tests only): callables or sequences giving, for the i-th HELLO
        this acceptor ever sees, its 32-byte short-term secret and its 64 bytes of Curve.random()
        draws (cookie nonce 16, cookie key 32, WELCOME nonce 16)."""
        ident = bytes(identity or b"")
        super().__init__("cz_acceptor", bytes(secret_key), socket_type, ident or None, len(ident), max_pending, device)
        self.socket_type = socket_type
        self.device = device
        self._secrets, self._entropy, self._seen = ephemeral_secrets, entropy, 0

    def hello(self, cmds):
        """N HELLO command bodies -> [(rc, event, slot, reply)]: reply is the WELCOME (slot >= 0), the
        ERROR command (box did not open: rc 0, event CRYPTOGRAPHIC, slot -1) or b"" (malformed)."""
        n = len(cmds)
        sec = self._injected(self._secrets, self._seen, n, 32)
        ent = self._injected(self._entropy, self._seen, n, 64)
        out = self._stage("hello", n, self._commands(cmds), HELLO_REPLY, (sec, ent))
        self._seen += n
        return out

    def initiate(self, slots, cmds):
        """N INITIATE command bodies for pending slots -> [(rc, event, slot, reply)]: reply is READY."""
        return self._stage("initiate", len(cmds), self._commands(cmds, slots), INITIATE_REPLY)

    def client_key(self, slot):
        k = ctypes.create_string_buffer(32)
        self._call("client_key", self._h, slot, k)
        return k.raw

    def mechanism(self, slot, device=None):
        """The CONNECTED CurveServerMechanism of an accepted slot (one connection at a time; many
        connections go to CurveBatchEngine.add_accepted)."""
        precom, n, pn = self.session(slot)
        return CurveServerMechanism(precom, cn_nonce=n, cn_peer_nonce=pn,
                                    device=self.device if device is None else device)
