"""Batching CURVE engine over the C-ABI (cz_engine_*): the StreamEngine encode/decode
loops (StreamEngine.java:379-535, :1052-1098) for many connections at once, with one
device batch per flush and socket-ready ZMTP v2 wire streams per connection.

    eng = CurveBatchEngine(arena_bytes=1 << 26)
    c = eng.add_connection(precom, as_server=False)          # CurveClientMechanism state
    ids = eng.add_accepted_many(acceptor, slots)              # N finished handshakes, one device chain
    eng.send(c, b"payload", more=False)
    eng.publish([c, c2, c3], b"payload")                      # one payload to many (PUB fan-out)
    eng.flush_out(); wire = eng.wire_out(c)                   # bytes for the socket
    eng.recv(c, received_bytes); eng.flush_in()
    for payload, flags in eng.messages_in(c): ...
    eng.error(c)                                              # (CZ_EPROTO, ZMTP event) after a failure
    eng.forward(a, b); eng.recv(a, received_bytes)            # a broker's route: what a receives leaves for b,
    eng.flush_forward(); wire = eng.forward_out(a)            # re-sealed in place, without delivery
"""
import ctypes

import numpy as np

from . import _lib


class _IOVEC(ctypes.Structure):
    _fields_ = [("base", ctypes.c_void_p), ("len", ctypes.c_uint64)]


class CurveBatchEngine:
    def __init__(self, arena_bytes=1 << 26, device=0):
        self._L = _lib.lib()
        h = ctypes.c_void_p()
        _lib.check(self._L.cz_engine_create(ctypes.byref(h), arena_bytes, device), "cz_engine_create")
        self._h = h

    def close(self):
        if self._h:
            self._L.cz_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_session(self, handshake):
        """A connection from a completed CURVE handshake (jeromq_amd.handshake): its cnPrecom and nonces."""
        rc = self._L.cz_engine_add_session(self._h, handshake._h)
        if rc < 0:
            _lib.check(rc, "cz_engine_add_session")
        return rc

    def add_accepted(self, acceptor, slot):
        """A connection from a slot the batched acceptor (jeromq_amd.acceptor) has accepted."""
        rc = self._L.cz_engine_add_accepted(self._h, acceptor._h, slot)
        if rc < 0:
            _lib.check(rc, "cz_engine_add_accepted")
        return rc

    def add_connected(self, connector, slot):
        """A connection from a slot the batched connector (jeromq_amd.connector) has connected."""
        rc = self._L.cz_engine_add_connected(self._h, connector._h, slot)
        if rc < 0:
            _lib.check(rc, "cz_engine_add_connected")
        return rc

    def add_connection(self, precom, as_server=False, cn_nonce=None, cn_peer_nonce=None):
        """Per-connection CURVE state after the handshake: client MESSAGEs start at nonce 3
        and expect the server's from 2 (cn_peer_nonce 1); the server the other way round."""
        if cn_nonce is None:
            cn_nonce = 2 if as_server else 3
        if cn_peer_nonce is None:
            cn_peer_nonce = 2 if as_server else 1
        k = (ctypes.c_uint8 * 32).from_buffer_copy(bytes(precom))
        rc = self._L.cz_engine_add_conn(self._h, 1 if as_server else 0, k, cn_nonce, cn_peer_nonce)
        if rc < 0:
            _lib.check(rc, "cz_engine_add_conn")
        return rc

    def remove_connection(self, conn):
        """The connection is gone (StreamEngine teardown): queued messages and received bytes are
        dropped, its subkeys wiped, and its id reused by a later add_connection."""
        _lib.check(self._L.cz_engine_remove_conn(self._h, conn), "cz_engine_remove_conn")

    # ---- bulk session hand-over: N sessions per call, one device chain whatever N is ----

    def add_connections(self, precoms, as_server=False, cn_nonce=None, cn_peer_nonce=None):
        """add_connection for many sessions at once -> [id]: the ids a loop of add_connection would
        return.  as_server: one flag for all or one per session; cn_nonce / cn_peer_nonce: None (the
        defaults of add_connection per role), one value for all or one per session."""
        keys = [bytes(k) for k in precoms]
        n = len(keys)
        if any(len(k) != 32 for k in keys):
            raise ValueError("every precom is 32 bytes")
        roles = [bool(as_server)] * n if isinstance(as_server, (bool, int)) else [bool(r) for r in as_server]

        def per_item(v, server_default, client_default):
            if v is None:
                return [server_default if r else client_default for r in roles]
            return [int(v)] * n if isinstance(v, int) else [int(x) for x in v]
        nonce, peer = per_item(cn_nonce, 2, 3), per_item(cn_peer_nonce, 2, 1)
        if not (len(roles) == len(nonce) == len(peer) == n):
            raise ValueError("one role and one nonce pair per precom")
        if n == 0:
            return []
        ids = np.empty(n, dtype=np.int32)
        rc = self._L.cz_engine_add_conns(self._h, n, np.array(roles, dtype=np.uint8).ctypes.data_as(ctypes.c_void_p),
                                         b"".join(keys), np.array(nonce, dtype=np.uint64).ctypes.data_as(ctypes.c_void_p),
                                         np.array(peer, dtype=np.uint64).ctypes.data_as(ctypes.c_void_p),
                                         ids.ctypes.data_as(ctypes.c_void_p))
        _lib.check(rc, "cz_engine_add_conns")
        return ids.tolist()

    def _add_many(self, fn, handshake, slots):
        arr = np.array(list(slots), dtype=np.int32)
        if len(arr) == 0:
            return []
        ids = np.empty(len(arr), dtype=np.int32)
        _lib.check(getattr(self._L, fn)(self._h, handshake._h, len(arr), arr.ctypes.data_as(ctypes.c_void_p),
                                        ids.ctypes.data_as(ctypes.c_void_p)), fn)
        return ids.tolist()

    def add_accepted_many(self, acceptor, slots):
        """add_accepted for many slots at once -> [id]; a slot without a completed handshake gives a
        negative entry (CZ_EINVAL), consumes no id and does not raise.  The session keys are read from
        the acceptor's device state; the slots may be released as soon as this returns."""
        return self._add_many("cz_engine_add_accepted_batch", acceptor, slots)

    def add_connected_many(self, connector, slots):
        """add_connected for many slots at once -> [id], as add_accepted_many."""
        return self._add_many("cz_engine_add_connected_batch", connector, slots)

    def remove_connections(self, conns):
        """remove_connection for a list -> [rc]: CZ_OK, or CZ_EINVAL for an id that is unknown, already
        removed or named before in the list (the others are removed)."""
        arr = np.array(list(conns), dtype=np.int32)
        if len(arr) == 0:
            return []
        rcs = np.empty(len(arr), dtype=np.int32)
        _lib.check(self._L.cz_engine_remove_conns(self._h, len(arr), arr.ctypes.data_as(ctypes.c_void_p),
                                                  rcs.ctypes.data_as(ctypes.c_void_p)), "cz_engine_remove_conns")
        return rcs.tolist()

    def msg_alloc(self, n):
        """Pinned payload buffer in the engine arena (ZMQ_MSG_ALLOCATOR); a ctypes array or None."""
        p = self._L.cz_engine_msg_alloc(self._h, n)
        return None if not p else (ctypes.c_uint8 * n).from_address(p)

    def send(self, conn, payload, more=False, command=False):
        flags = (_lib.CZ_MSG_MORE if more else 0) | (_lib.CZ_MSG_COMMAND if command else 0)
        if isinstance(payload, ctypes.Array):
            ptr, n = ctypes.addressof(payload), ctypes.sizeof(payload)
        else:
            b = bytes(payload)
            buf = ctypes.create_string_buffer(b, len(b)) if b else None
            ptr, n = (ctypes.addressof(buf) if buf else None), len(b)
        return self._L.cz_engine_send(self._h, conn, ptr, n, flags)

    def publish(self, conns, payload, more=False, command=False):
        """PUB fan-out (Dist.distribute): queue the one payload for every connection in `conns`, in
        list order; it is staged in the arena once.  Connections that have failed are skipped.
        Returns the number of frames queued; an unknown id, an over-long payload or a full arena
        raises with nothing queued."""
        flags = (_lib.CZ_MSG_MORE if more else 0) | (_lib.CZ_MSG_COMMAND if command else 0)
        if isinstance(payload, ctypes.Array):
            ptr, n = ctypes.addressof(payload), ctypes.sizeof(payload)
        else:
            b = bytes(payload)
            buf = ctypes.create_string_buffer(b, len(b)) if b else None
            ptr, n = (ctypes.addressof(buf) if buf else None), len(b)
        ids = (ctypes.c_int * max(len(conns), 1))(*conns)
        queued = ctypes.c_uint32()
        _lib.check(self._L.cz_engine_publish(self._h, ids, len(conns), ptr, n, flags, ctypes.byref(queued)),
                   "cz_engine_publish")
        return queued.value

    def flush_out(self):
        _lib.check(self._L.cz_engine_flush_out(self._h), "cz_engine_flush_out")

    def wire_out(self, conn):
        p, n = ctypes.c_void_p(), ctypes.c_uint64()
        _lib.check(self._L.cz_engine_wire_out(self._h, conn, ctypes.byref(p), ctypes.byref(n)), "cz_engine_wire_out")
        return ctypes.string_at(p.value, n.value) if n.value else b""

    def wire_iov(self, conn):
        """The connection's stream as gather-write pieces [(address, length)] of the flush output."""
        cnt = ctypes.c_uint32()
        _lib.check(self._L.cz_engine_wire_iov(self._h, conn, None, 0, ctypes.byref(cnt)), "cz_engine_wire_iov")
        arr = (_IOVEC * max(cnt.value, 1))()
        _lib.check(self._L.cz_engine_wire_iov(self._h, conn, arr, cnt.value, ctypes.byref(cnt)), "cz_engine_wire_iov")
        return [(arr[k].base, arr[k].len) for k in range(cnt.value)]

    def recv(self, conn, wire):
        b = bytes(wire)
        buf = ctypes.create_string_buffer(b, len(b)) if b else None
        return self._L.cz_engine_recv(self._h, conn, buf, len(b))

    def recv_into(self, conn, read, max_bytes=1 << 20):
        """Zero-copy receive: `read(memoryview)` fills the engine's pinned buffer (e.g.
        sock.recv_into) and returns the byte count, which is committed."""
        p, n = ctypes.c_void_p(), ctypes.c_uint64()
        _lib.check(self._L.cz_engine_recv_buffer(self._h, conn, max_bytes, ctypes.byref(p), ctypes.byref(n)),
                   "cz_engine_recv_buffer")
        view = memoryview((ctypes.c_uint8 * n.value).from_address(p.value)).cast("B")
        got = read(view)
        _lib.check(self._L.cz_engine_recv_commit(self._h, conn, got), "cz_engine_recv_commit")
        return got

    def flush_in(self):
        _lib.check(self._L.cz_engine_flush_in(self._h), "cz_engine_flush_in")

    @property
    def fanin_frames(self):
        """Frames of the last flush_in that the fan-in open (cz_open_fanin_runs) took out of the segment
        plan: runs of at least 64 same-size frames with payloads up to cz_tune("fanin_short") bytes."""
        return int(self._L.cz_engine_fanin_frames(self._h))

    @property
    def fanin_split_frames(self):
        """Frames of the last flush_in that the split fan-in open (cz_open_fanin_split) took out of the
        segment plan: the other runs of at least 64 same-size frames with payloads of at least
        cz_tune("fanin_split") bytes (0: the rule is off)."""
        return int(self._L.cz_engine_fanin_split_frames(self._h))

    @property
    def scan_frames(self):
        """Frames of the last flush_in that the scanned path opened: parsed on the device (cz_v2_scan) and
        opened from the wire bytes where they lie.  The whole flush or nothing: cz_tune("scan_in") = n > 0,
        at least 64 connections with received bytes, none holding more than n."""
        return int(self._L.cz_engine_scan_frames(self._h))

    # ---- forward routes: a broker's Proxy.forward without the plaintext reaching memory ----

    def forward(self, from_, to):
        """Route everything `from_` receives to `to`, re-sealed (cz_engine_forward); to=-1 or None clears the
        route.  One source per destination; A -> B with B -> A is the normal proxy.  flush_in skips a routed
        connection: its bytes wait for flush_forward."""
        _lib.check(self._L.cz_engine_forward(self._h, from_, -1 if to is None else to), "cz_engine_forward")

    def flush_forward(self):
        """Re-seal every routed connection's received whole frames in place for its destination, in one device
        chain; what leaves is cut at the first rejected frame, which fails the source as flush_in would."""
        _lib.check(self._L.cz_engine_flush_forward(self._h), "cz_engine_flush_forward")

    def forward_out(self, conn):
        """The bytes the last flush_forward made of `conn`'s received stream: wire frames for the socket of its
        route's destination."""
        p, n = ctypes.c_void_p(), ctypes.c_uint64()
        _lib.check(self._L.cz_engine_forward_out(self._h, conn, ctypes.byref(p), ctypes.byref(n)),
                   "cz_engine_forward_out")
        return ctypes.string_at(p.value, n.value) if n.value else b""

    @property
    def forward_frames(self):
        """Frames the last flush_forward forwarded."""
        return int(self._L.cz_engine_forward_frames(self._h))

    def messages_in(self, conn):
        cnt = ctypes.c_uint32()
        _lib.check(self._L.cz_engine_msgs_in(self._h, conn, ctypes.byref(cnt)), "cz_engine_msgs_in")
        out = []
        p, n, fl = ctypes.c_void_p(), ctypes.c_uint32(), ctypes.c_int()
        for i in range(cnt.value):
            _lib.check(self._L.cz_engine_msg_in(self._h, conn, i, ctypes.byref(p), ctypes.byref(n), ctypes.byref(fl)),
                       "cz_engine_msg_in")
            out.append((ctypes.string_at(p.value, n.value) if n.value else b"", fl.value))
        return out

    def error(self, conn):
        ev = ctypes.c_int()
        rc = self._L.cz_engine_conn_error(self._h, conn, ctypes.byref(ev))
        return rc, ev.value

    def nonce(self, conn):
        return int(self._L.cz_engine_nonce(self._h, conn))

    def peer_nonce(self, conn):
        return int(self._L.cz_engine_peer_nonce(self._h, conn))
