"""Batched CURVE client handshake over the C-ABI (cz_connector_*): the client half of
CurveClientMechanism's handshake (CurveClientMechanism.java:246-429) for many connections per call.

    con = CurveConnector(public, secret, socket_type=ZMQ_DEALER, identity=b"collector", max_pending=1 << 16)
    for (rc, event, slot, hello), conn in zip(con.hello(server_keys), conns): ...   # N HELLO to send
    for (rc, event, slot, initiate), conn in zip(con.welcome(slots, welcomes), conns): ...
    for (rc, event, slot, _), conn in zip(con.ready(slots, readys), conns): ...
    c = engine.add_connected(con, slot)        # the session moves to the batching engine
    con.release(slot)
    ids = engine.add_connected_many(con, slots); con.release_many(slots)   # the same for many slots at once

Each stage is a fixed number of device launches and one synchronisation whatever the batch size
(jeromq_amd/csrc/cz_connector.cpp).  Every item behaves as one CurveClientHandshake fed the same
command; a slot that failed or received an ERROR takes no further command.  session, peer_property,
release, pending and close: _hs_batch.py.
"""
import ctypes

from ._hs_batch import _HsBatch
from .handshake import ZMQ_PAIR
from .mechanism import CurveClientMechanism

HELLO_REPLY = 200     # the HELLO command
WELCOME_REPLY = 513   # INITIATE: 113 + 16 + 128 + at most 256 bytes of metadata


class CurveConnector(_HsBatch):
    def __init__(self, public_key, secret_key, socket_type=ZMQ_PAIR, identity=b"", max_pending=1024, device=0,
                 ephemeral_secrets=None, vouch_nonces=None):
        """ephemeral_secrets / vouch_nonces (tests only): callables or sequences giving, for the i-th
        connection this connector ever dials, its 32-byte short-term secret, and for the i-th command
        it is ever given in welcome(), the 16 random bytes of the vouch nonce."""
        ident = bytes(identity or b"")
        super().__init__("cz_connector", bytes(public_key), bytes(secret_key), socket_type, ident or None, len(ident),
                         max_pending, device)
        self.socket_type = socket_type
        self.device = device
        self._secrets, self._vnonces, self._dialled, self._welcomed = ephemeral_secrets, vouch_nonces, 0, 0

    def hello(self, server_keys):
        """N server keys (one per connection to open) -> [(rc, event, slot, HELLO)]; rc CZ_EAGAIN and
        slot -1 when the table is full."""
        n = len(server_keys)
        keys = b"".join(bytes(k) for k in server_keys)
        if len(keys) != 32 * n:
            raise ValueError("server keys are 32 bytes each")
        sec = self._injected(self._secrets, self._dialled, n, 32)
        out = self._stage("hello", n, [keys], HELLO_REPLY, (sec,))
        self._dialled += n
        return out

    def welcome(self, slots, cmds):
        """N command bodies (WELCOME, or ERROR) for slots that sent HELLO -> [(rc, event, slot, reply)]:
        reply is the INITIATE, or b"" when the item failed or was an ERROR command."""
        n = len(cmds)
        args = self._commands(cmds, slots)
        ent = self._injected(self._vnonces, self._welcomed, n, 16)
        out = self._stage("welcome", n, args, WELCOME_REPLY, (ent,))
        self._welcomed += n
        return out

    def ready(self, slots, cmds):
        """N command bodies (READY, or ERROR) for slots that sent INITIATE -> [(rc, event, slot, b"")];
        rc 0 with error_status(slot) == 0 and a session: the connection is up."""
        return self._stage("ready", len(cmds), self._commands(cmds, slots))

    def error_status(self, slot):
        """the status code (300 / 400 / 500) of a well-formed ERROR command the slot received, else 0"""
        return int(self._L.cz_connector_error_status(self._h, slot))

    def server_key(self, slot):
        k = ctypes.create_string_buffer(32)
        self._call("server_key", self._h, slot, k)
        return k.raw

    def mechanism(self, slot, device=None):
        """The CONNECTED CurveClientMechanism of a connected slot (one connection at a time; many
        connections go to CurveBatchEngine.add_connected)."""
        precom, n, pn = self.session(slot)
        return CurveClientMechanism(precom, cn_nonce=n, cn_peer_nonce=pn,
                                    device=self.device if device is None else device)
