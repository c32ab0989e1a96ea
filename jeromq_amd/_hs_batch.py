"""What CurveAcceptor (acceptor.py) and CurveConnector (connector.py) share over the C-ABI: the handle's
life, the shape of a stage call and the calls both sides have under their own prefix (cz_acceptor_* /
cz_connector_*), as the two share their host core in C (jeromq_amd/csrc/cz_hs_batch.h)."""
import ctypes

import numpy as np

from . import _lib


def _pack(cmds):
    """command bodies -> (one buffer, offsets, sizes)"""
    cmds = [bytes(c) for c in cmds]
    size = np.array([len(c) for c in cmds], dtype=np.uint32)
    off = np.zeros(len(cmds), dtype=np.uint64)
    if len(cmds) > 1:
        off[1:] = np.cumsum(size[:-1], dtype=np.uint64)
    return b"".join(cmds), off, size


class _HsBatch:
    def __init__(self, prefix, *create_args):
        """prefix: "cz_acceptor" or "cz_connector"; create_args: what <prefix>_create takes after the handle"""
        self._L = _lib.lib()
        self._prefix = prefix
        h = ctypes.c_void_p()
        self._call("create", ctypes.byref(h), *create_args)
        self._h = h

    def _call(self, name, *args):
        fn = f"{self._prefix}_{name}"
        _lib.check(getattr(self._L, fn)(*args), fn)

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._L, self._prefix + "_destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _injected(src, first, count, width):
        """`count` test values of `width` bytes from a callable or a sequence, starting at index `first`"""
        if src is None:
            return None
        out = b"".join(bytes(src(first + i) if callable(src) else src[first + i]) for i in range(count))
        if len(out) != count * width:
            raise ValueError(f"injected values must be {width} bytes each")
        return out

    @staticmethod
    def _commands(cmds, slots=None):
        """the C arguments for N command bodies: [slots,] buffer, its size, offsets, sizes"""
        buf, off, size = _pack(cmds)
        args = [buf, len(buf), off.ctypes.data_as(ctypes.c_void_p), size.ctypes.data_as(ctypes.c_void_p)]
        if slots is None:
            return args
        if len(slots) != len(cmds):
            raise ValueError("one slot per command")
        return [np.array(list(slots), dtype=np.int32).ctypes.data_as(ctypes.c_void_p)] + args

    @staticmethod
    def _results(res, reply=None, stride=0):
        return [(r.rc, r.event & 0xffffffff, r.slot, reply.raw[i * stride:i * stride + r.reply_len] if reply is not None else b"")
                for i, r in enumerate(res)]

    def _stage(self, name, n, args, reply_stride=0, test_values=()):
        """<prefix>_<name>(handle, n, *args, [reply, reply_stride,] results, *test_values) -> [(rc, event, slot, reply)]"""
        res = (_lib.cz_accept_result * max(n, 1))()
        reply = ctypes.create_string_buffer(max(n, 1) * reply_stride) if reply_stride else None
        self._call(name, self._h, n, *args, *((reply, reply_stride) if reply_stride else ()), res, *test_values)
        return self._results(res[:n], reply, reply_stride)

    def session(self, slot):
        """(cnPrecom, cn_nonce, cn_peer_nonce) of a slot whose handshake completed"""
        k = ctypes.create_string_buffer(32)
        n, pn = ctypes.c_uint64(), ctypes.c_uint64()
        self._call("session", self._h, slot, k, ctypes.byref(n), ctypes.byref(pn))
        return k.raw, n.value, pn.value

    def peer_property(self, slot, name):
        v, n = ctypes.c_void_p(), ctypes.c_uint32()
        if getattr(self._L, self._prefix + "_peer_property")(self._h, slot, name.encode(), ctypes.byref(v),
                                                             ctypes.byref(n)) != _lib.CZ_OK:
            return None
        return ctypes.string_at(v, n.value) if n.value else b""

    def release(self, slot):
        self._call("release", self._h, slot)

    def release_many(self, slots):
        """release() for a list, all or nothing: one device launch wipes every slot's record.  A slot
        that is not in use or is named twice raises with nothing released."""
        arr = np.array(list(slots), dtype=np.int32)
        self._call("release_batch", self._h, len(arr), arr.ctypes.data_as(ctypes.c_void_p))

    def pending(self):
        return int(getattr(self._L, self._prefix + "_pending")(self._h))
