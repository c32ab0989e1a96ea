"""ZMTP v2 framing (zmq/io/coder/v2/V2Encoder.java, V2Decoder.java) over the C-ABI.

`parse` is the host V2Decoder walk (one header per frame, no device needed);
`copy` launches the device pack/unpack kernel (k_v2_copy) that moves bodies
between aligned slots and socket-ready wire streams; `scan` / `scan_emit` parse
many received streams where they lie in device memory, one lane per stream
(k_v2_scan, k_v2_place, k_v2_emit).
"""
import ctypes

import numpy as np

from . import _lib

V2_FRAME_DTYPE = np.dtype([("body_off", "<u8"), ("size", "<u4"), ("msg_flags", "<u4")])
V2_ITEM_DTYPE = np.dtype([("src_off", "<u8"), ("dst_off", "<u8"), ("size", "<u4"), ("flags", "<u4")])
V2_STREAM_DTYPE = np.dtype([("off", "<u8"), ("len", "<u8"), ("floor", "<u8"), ("key_idx", "<u4"), ("reserved", "<u4")])
V2_STREAM_RESULT_DTYPE = np.dtype([("consumed", "<u8"), ("slot_off", "<u8"), ("first", "<u4"), ("nframes", "<u4"),
                                   ("rc", "<i4"), ("reserved", "<u4")])
V2_TOTALS_DTYPE = np.dtype([("nframes", "<u8"), ("slot_bytes", "<u8")])
assert V2_STREAM_DTYPE.itemsize == 32 and V2_STREAM_RESULT_DTYPE.itemsize == 32 and V2_TOTALS_DTYPE.itemsize == 16


def header_size(size):
    """2, or 9 when the body exceeds 255 bytes (V2Encoder.java:33-55)."""
    return int(_lib.lib().cz_v2_header_size(size))


def parse(wire, maxmsgsize=-1, cap=None):
    """Parse whole frames of `wire` (bytes-like).  Returns (frames, consumed, rc): frames is a
    V2_FRAME_DTYPE array, consumed the bytes of whole frames, rc CZ_OK / CZ_EPROTO / CZ_EMSGSIZE
    for a bad header after the returned frames (V2Decoder.java:52-58, Decoder.java:76-98)."""
    buf = np.frombuffer(bytes(wire), dtype=np.uint8)
    if cap is None:
        cap = len(buf) // 2 + 1
    frames = np.zeros(max(cap, 1), dtype=V2_FRAME_DTYPE)
    nf, consumed = ctypes.c_uint32(), ctypes.c_uint64()
    rc = _lib.lib().cz_v2_parse(buf.ctypes.data if len(buf) else None, len(buf), maxmsgsize, frames.ctypes.data,
                                cap, ctypes.byref(nf), ctypes.byref(consumed))
    return frames[:nf.value], consumed.value, rc


def copy(items, src, dst, stream=None):
    """Device pack/unpack: items = device tensor of V2_ITEM_DTYPE records (24 B each)."""
    from .batch import _ptr, _stream
    count = items.numel() // V2_ITEM_DTYPE.itemsize
    _lib.check(_lib.lib().cz_v2_copy(_ptr(items), count, _ptr(src), _ptr(dst), _stream(stream)), "cz_v2_copy")


def to_device(records, device):
    """A numpy record array as a uint8 device tensor (at least one byte long, so it has an address)."""
    import torch
    raw = np.ascontiguousarray(records).view(np.uint8).reshape(-1)
    t = torch.zeros(max(raw.size, 1), dtype=torch.uint8, device=device)
    if raw.size:
        t[:raw.size] = torch.from_numpy(raw.copy()).to(device)
    return t


def scan(streams, wire, maxmsgsize=-1, slot_align=128, results=None, totals=None, stream=None):
    """Device parse of many received streams (cz_v2_scan): `streams` is a V2_STREAM_DTYPE array (uploaded
    here) or a device tensor of such records, `wire` the device tensor the streams lie in.  One lane
    per stream walks the headers with `parse`'s rules.  Returns (results, totals): device uint8 tensors
    holding one V2_STREAM_RESULT_DTYPE record per stream and the V2_TOTALS_DTYPE record; pass your
    own to have them written in place.  Asynchronous on `stream`."""
    import torch
    from .batch import _ptr, _stream
    if isinstance(streams, np.ndarray):
        streams = to_device(streams.astype(V2_STREAM_DTYPE, copy=False), wire.device)
    count = streams.numel() // V2_STREAM_DTYPE.itemsize
    if results is None:
        results = torch.zeros(max(count, 1) * V2_STREAM_RESULT_DTYPE.itemsize, dtype=torch.uint8, device=wire.device)
    if totals is None:
        totals = torch.zeros(V2_TOTALS_DTYPE.itemsize, dtype=torch.uint8, device=wire.device)
    _lib.check(_lib.lib().cz_v2_scan(_ptr(streams), count, _ptr(wire), maxmsgsize, slot_align, _ptr(results),
                                     _ptr(totals), _stream(stream)), "cz_v2_scan")
    return results, totals


def scan_emit(streams, results, wire, slot_align=128, frames=None, desc=None, stream=None):
    """The records of the frames `scan` counted (cz_v2_scan_emit): frame k of stream s at index
    results[s].first + k of `frames` (V2_FRAME_DTYPE, body_off relative to the stream) and / or `desc`
    (cz_frame_desc for open_batch with in = wire).  Device tensors sized by the scan's totals; either
    may be None."""
    from .batch import _ptr, _stream
    if isinstance(streams, np.ndarray):
        streams = to_device(streams.astype(V2_STREAM_DTYPE, copy=False), wire.device)
    count = streams.numel() // V2_STREAM_DTYPE.itemsize
    _lib.check(_lib.lib().cz_v2_scan_emit(_ptr(streams), _ptr(results), count, _ptr(wire), slot_align, _ptr(frames),
                                          _ptr(desc), _stream(stream)), "cz_v2_scan_emit")
