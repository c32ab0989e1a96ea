"""Batched CURVE server handshake over the C-ABI (cz_acceptor_*): the server half of
CurveServerMechanism's handshake (CurveServerMechanism.java:254-517) for many connections per call.

    acc = CurveAcceptor(server_secret, socket_type=ZMQ_ROUTER, max_pending=1 << 16)
    for (rc, event, slot, welcome), conn in zip(acc.hello(hellos), conns): ...   # N HELLO -> N WELCOME
    for (rc, event, slot, ready), conn in zip(acc.initiate(slots, initiates), conns): ...
    acc.client_key(slot)                       # allow-list check before READY is sent
    c = engine.add_accepted(acc, slot)         # the session moves to the batching engine
    acc.release(slot)

Each stage is a fixed number of device launches and one synchronisation whatever the batch size
(jeromq_amd/csrc/cz_acceptor.cpp).  Every item behaves as one CurveServerHandshake fed the same
command.  ZAP is out of scope.
"""
import ctypes

import numpy as np

from . import _lib
from .handshake import ZMQ_PAIR
from .mechanism import CurveServerMechanism

HELLO_REPLY = 168     # the WELCOME command
INITIATE_REPLY = 288  # READY: 14 + 16 + at most 256 bytes of metadata, rounded up


def _pack(cmds):
    """command bodies -> (one buffer, offsets, sizes)"""
    cmds = [bytes(c) for c in cmds]
    size = np.array([len(c) for c in cmds], dtype=np.uint32)
    off = np.zeros(len(cmds), dtype=np.uint64)
    if len(cmds) > 1:
        off[1:] = np.cumsum(size[:-1], dtype=np.uint64)
    return b"".join(cmds), off, size


class CurveAcceptor:
    def __init__(self, secret_key, socket_type=ZMQ_PAIR, identity=b"", max_pending=1024, device=0,
                 ephemeral_secrets=None, entropy=None):
        """ephemeral_secrets / entropy (tests only): callables or sequences giving, for the i-th HELLO
        this acceptor ever sees, its 32-byte short-term secret and its 64 bytes of Curve.random()
        draws (cookie nonce 16, cookie key 32, WELCOME nonce 16)."""
        self._L = _lib.lib()
        h = ctypes.c_void_p()
        ident = bytes(identity or b"")
        rc = self._L.cz_acceptor_create(ctypes.byref(h), bytes(secret_key), socket_type, ident or None, len(ident),
                                        max_pending, device)
        _lib.check(rc, "cz_acceptor_create")
        self._h = h
        self.socket_type = socket_type
        self.device = device
        self._secrets, self._entropy, self._seen = ephemeral_secrets, entropy, 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.cz_acceptor_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _injected(self, src, count, width):
        if src is None:
            return None
        out = b"".join(bytes(src(self._seen + i) if callable(src) else src[self._seen + i]) for i in range(count))
        if len(out) != count * width:
            raise ValueError(f"injected values must be {width} bytes each")
        return out

    @staticmethod
    def _results(res, reply, stride):
        return [(r.rc, r.event & 0xffffffff, r.slot, reply.raw[i * stride:i * stride + r.reply_len])
                for i, r in enumerate(res)]

    def hello(self, cmds):
        """N HELLO command bodies -> [(rc, event, slot, reply)]: reply is the WELCOME (slot >= 0), the
        ERROR command (box did not open: rc 0, event CRYPTOGRAPHIC, slot -1) or b"" (malformed)."""
        n = len(cmds)
        buf, off, size = _pack(cmds)
        res = (_lib.cz_accept_result * max(n, 1))()
        reply = ctypes.create_string_buffer(max(n, 1) * HELLO_REPLY)
        sec = self._injected(self._secrets, n, 32)
        ent = self._injected(self._entropy, n, 64)
        rc = self._L.cz_acceptor_hello(self._h, n, buf, len(buf), off.ctypes.data, size.ctypes.data, reply,
                                       HELLO_REPLY, res, sec, ent)
        _lib.check(rc, "cz_acceptor_hello")
        self._seen += n
        return self._results(res[:n], reply, HELLO_REPLY)

    def initiate(self, slots, cmds):
        """N INITIATE command bodies for pending slots -> [(rc, event, slot, reply)]: reply is READY."""
        n = len(cmds)
        if len(slots) != n:
            raise ValueError("one slot per command")
        buf, off, size = _pack(cmds)
        sl = np.array(list(slots), dtype=np.int32)
        res = (_lib.cz_accept_result * max(n, 1))()
        reply = ctypes.create_string_buffer(max(n, 1) * INITIATE_REPLY)
        rc = self._L.cz_acceptor_initiate(self._h, n, sl.ctypes.data, buf, len(buf), off.ctypes.data,
                                          size.ctypes.data, reply, INITIATE_REPLY, res)
        _lib.check(rc, "cz_acceptor_initiate")
        return self._results(res[:n], reply, INITIATE_REPLY)

    def session(self, slot):
        """(cnPrecom, cn_nonce, cn_peer_nonce) of an accepted slot"""
        k = ctypes.create_string_buffer(32)
        n, pn = ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(self._L.cz_acceptor_session(self._h, slot, k, ctypes.byref(n), ctypes.byref(pn)),
                   "cz_acceptor_session")
        return k.raw, n.value, pn.value

    def client_key(self, slot):
        k = ctypes.create_string_buffer(32)
        _lib.check(self._L.cz_acceptor_client_key(self._h, slot, k), "cz_acceptor_client_key")
        return k.raw

    def peer_property(self, slot, name):
        v, n = ctypes.c_void_p(), ctypes.c_uint32()
        if self._L.cz_acceptor_peer_property(self._h, slot, name.encode(), ctypes.byref(v),
                                             ctypes.byref(n)) != _lib.CZ_OK:
            return None
        return ctypes.string_at(v, n.value) if n.value else b""

    def mechanism(self, slot, device=None):
        """The CONNECTED CurveServerMechanism of an accepted slot (one connection at a time; many
        connections go to CurveBatchEngine.add_accepted)."""
        precom, n, pn = self.session(slot)
        return CurveServerMechanism(precom, cn_nonce=n, cn_peer_nonce=pn,
                                    device=self.device if device is None else device)

    def release(self, slot):
        _lib.check(self._L.cz_acceptor_release(self._h, slot), "cz_acceptor_release")

    def pending(self):
        return int(self._L.cz_acceptor_pending(self._h))
