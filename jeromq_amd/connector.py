"""Batched CURVE client handshake over the C-ABI (cz_connector_*): the client half of
CurveClientMechanism's handshake (CurveClientMechanism.java:246-429) for many connections per call.

    con = CurveConnector(public, secret, socket_type=ZMQ_DEALER, identity=b"collector", max_pending=1 << 16)
    for (rc, event, slot, hello), conn in zip(con.hello(server_keys), conns): ...   # N HELLO to send
    for (rc, event, slot, initiate), conn in zip(con.welcome(slots, welcomes), conns): ...
    for (rc, event, slot, _), conn in zip(con.ready(slots, readys), conns): ...
    c = engine.add_connected(con, slot)        # the session moves to the batching engine
    con.release(slot)

Each stage is a fixed number of device launches and one synchronisation whatever the batch size
(jeromq_amd/csrc/cz_connector.cpp).  Every item behaves as one CurveClientHandshake fed the same
command; a slot that failed or received an ERROR takes no further command.
"""
import ctypes

import numpy as np

from . import _lib
from .acceptor import _pack
from .handshake import ZMQ_PAIR
from .mechanism import CurveClientMechanism

HELLO_REPLY = 200     # the HELLO command
WELCOME_REPLY = 513   # INITIATE: 113 + 16 + 128 + at most 256 bytes of metadata


class CurveConnector:
    def __init__(self, public_key, secret_key, socket_type=ZMQ_PAIR, identity=b"", max_pending=1024, device=0,
                 ephemeral_secrets=None, vouch_nonces=None):
        """ephemeral_secrets / vouch_nonces (tests only): callables or sequences giving, for the i-th
        connection this connector ever dials, its 32-byte short-term secret, and for the i-th command
        it is ever given in welcome(), the 16 random bytes of the vouch nonce."""
        self._L = _lib.lib()
        h = ctypes.c_void_p()
        ident = bytes(identity or b"")
        rc = self._L.cz_connector_create(ctypes.byref(h), bytes(public_key), bytes(secret_key), socket_type,
                                         ident or None, len(ident), max_pending, device)
        _lib.check(rc, "cz_connector_create")
        self._h = h
        self.socket_type = socket_type
        self.device = device
        self._secrets, self._vnonces, self._dialled, self._welcomed = ephemeral_secrets, vouch_nonces, 0, 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.cz_connector_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _injected(src, first, count, width):
        if src is None:
            return None
        out = b"".join(bytes(src(first + i) if callable(src) else src[first + i]) for i in range(count))
        if len(out) != count * width:
            raise ValueError(f"injected values must be {width} bytes each")
        return out

    @staticmethod
    def _results(res, reply=None, stride=0):
        return [(r.rc, r.event & 0xffffffff, r.slot, reply.raw[i * stride:i * stride + r.reply_len] if reply is not None else b"")
                for i, r in enumerate(res)]

    def hello(self, server_keys):
        """N server keys (one per connection to open) -> [(rc, event, slot, HELLO)]; rc CZ_EAGAIN and
        slot -1 when the table is full."""
        n = len(server_keys)
        keys = b"".join(bytes(k) for k in server_keys)
        if len(keys) != 32 * n:
            raise ValueError("server keys are 32 bytes each")
        res = (_lib.cz_accept_result * max(n, 1))()
        reply = ctypes.create_string_buffer(max(n, 1) * HELLO_REPLY)
        sec = self._injected(self._secrets, self._dialled, n, 32)
        rc = self._L.cz_connector_hello(self._h, n, keys, reply, HELLO_REPLY, res, sec)
        _lib.check(rc, "cz_connector_hello")
        self._dialled += n
        return self._results(res[:n], reply, HELLO_REPLY)

    def welcome(self, slots, cmds):
        """N command bodies (WELCOME, or ERROR) for slots that sent HELLO -> [(rc, event, slot, reply)]:
        reply is the INITIATE, or b"" when the item failed or was an ERROR command."""
        n = len(cmds)
        if len(slots) != n:
            raise ValueError("one slot per command")
        buf, off, size = _pack(cmds)
        sl = np.array(list(slots), dtype=np.int32)
        res = (_lib.cz_accept_result * max(n, 1))()
        reply = ctypes.create_string_buffer(max(n, 1) * WELCOME_REPLY)
        ent = self._injected(self._vnonces, self._welcomed, n, 16)
        rc = self._L.cz_connector_welcome(self._h, n, sl.ctypes.data, buf, len(buf), off.ctypes.data,
                                          size.ctypes.data, reply, WELCOME_REPLY, res, ent)
        _lib.check(rc, "cz_connector_welcome")
        self._welcomed += n
        return self._results(res[:n], reply, WELCOME_REPLY)

    def ready(self, slots, cmds):
        """N command bodies (READY, or ERROR) for slots that sent INITIATE -> [(rc, event, slot, b"")];
        rc 0 with error_status(slot) == 0 and a session: the connection is up."""
        n = len(cmds)
        if len(slots) != n:
            raise ValueError("one slot per command")
        buf, off, size = _pack(cmds)
        sl = np.array(list(slots), dtype=np.int32)
        res = (_lib.cz_accept_result * max(n, 1))()
        rc = self._L.cz_connector_ready(self._h, n, sl.ctypes.data, buf, len(buf), off.ctypes.data,
                                        size.ctypes.data, res)
        _lib.check(rc, "cz_connector_ready")
        return self._results(res[:n])

    def session(self, slot):
        """(cnPrecom, cn_nonce, cn_peer_nonce) of a connected slot"""
        k = ctypes.create_string_buffer(32)
        n, pn = ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(self._L.cz_connector_session(self._h, slot, k, ctypes.byref(n), ctypes.byref(pn)),
                   "cz_connector_session")
        return k.raw, n.value, pn.value

    def peer_property(self, slot, name):
        v, n = ctypes.c_void_p(), ctypes.c_uint32()
        if self._L.cz_connector_peer_property(self._h, slot, name.encode(), ctypes.byref(v),
                                              ctypes.byref(n)) != _lib.CZ_OK:
            return None
        return ctypes.string_at(v, n.value) if n.value else b""

    def error_status(self, slot):
        """the status code (300 / 400 / 500) of a well-formed ERROR command the slot received, else 0"""
        return int(self._L.cz_connector_error_status(self._h, slot))

    def server_key(self, slot):
        k = ctypes.create_string_buffer(32)
        _lib.check(self._L.cz_connector_server_key(self._h, slot, k), "cz_connector_server_key")
        return k.raw

    def mechanism(self, slot, device=None):
        """The CONNECTED CurveClientMechanism of a connected slot (one connection at a time; many
        connections go to CurveBatchEngine.add_connected)."""
        precom, n, pn = self.session(slot)
        return CurveClientMechanism(precom, cn_nonce=n, cn_peer_nonce=pn,
                                    device=self.device if device is None else device)

    def release(self, slot):
        _lib.check(self._L.cz_connector_release(self._h, slot), "cz_connector_release")

    def pending(self):
        return int(self._L.cz_connector_pending(self._h))
